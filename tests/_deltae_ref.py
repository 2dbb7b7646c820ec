"""NumPy-only restatement of the colour difference of include/sr_hip.h: scikit-image 0.18.3's rgb2lab of a uint8 image and its
deltaE_ciede2000 (kL = kC = kH = 1) / deltaE_cie76, in float64, plus the record (count, sum, sum2, max, histogram of 1/16-wide
bins), the percentile and fraction rules and the per-cell form.  The main interpreter has no scikit-image: tests/test_deltae_host.py
holds this file to tests/golden/deltae_skimage.npz (scikit-image's own values) at 1e-12 absolute, and it then serves the shapes
the fixture does not hold.

MUTANTS names deliberate one-term errors (`mutant=`); each must leave the fixture's bars (tests/test_deltae_host.py)."""
from fractions import Fraction

import numpy as np

CIEDE2000, CIE76 = 0, 1
BINS = 2048
M = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))
WHITE = (0.95047, 1.0, 1.08883)
MUTANTS = ("nonstrict_pi", "hsum_branch", "pow_25_6", "centre_270", "white_d50", "no_chroma_gain")
# "hbar_halved" (Hbar halved where a chroma is 0, where it must be the sum) is understood too, but it is NOT a mutant that any
# input can tell apart: where C1' C2' == 0 the hue term is 2 sqrt(0) sin(.) = 0, and Hbar reaches the result only through
# H_term and R = ... H_term.  tests/test_deltae_host.py asserts exactly that.


def table():
    v = np.arange(256, dtype=np.float64) / 255.0
    out = v / 12.92
    m = v > 0.04045
    out[m] = np.power((v[m] + 0.055) / 1.055, 2.4)
    return out


def to_rgb(img):
    """h x w (gray: R = G = B), h x w x 1, h x w x 3 or h x w x 4 (alpha ignored) -> h x w x 3."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[..., None]
    if img.shape[2] == 1:
        return np.repeat(img, 3, axis=2)
    return img[..., :3]


def rgb2lab(img, mutant=None):
    lin = table()[to_rgb(img)]
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    white = (0.9642, 1.0, 0.8251) if mutant == "white_d50" else WHITE
    f = []
    for row, wp in zip(M, white):
        t = ((row[0] * r + row[1] * g) + row[2] * b) / wp
        f.append(np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0))
    fx, fy, fz = f
    return np.stack([116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)], axis=-1)


def cie76(lab1, lab2):
    d = np.asarray(lab2, np.float64) - np.asarray(lab1, np.float64)
    return np.sqrt((d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2)


def ciede2000(lab1, lab2, mutant=None, parts=False):
    lab1, lab2 = np.asarray(lab1, np.float64), np.asarray(lab2, np.float64)
    L1, a1, b1 = lab1[..., 0], lab1[..., 1], lab1[..., 2]
    L2, a2, b2 = lab2[..., 0], lab2[..., 1], lab2[..., 2]
    pi, two_pi = np.pi, 2 * np.pi
    p25 = 25.0 ** (6 if mutant == "pow_25_6" else 7)
    cbar = 0.5 * (np.hypot(a1, b1) + np.hypot(a2, b2))
    c7 = cbar ** 7
    scale = 1 + 0.5 * (1 - np.sqrt(c7 / (c7 + p25)))
    if mutant == "no_chroma_gain":
        scale = np.ones_like(scale)

    def polar(x, y):
        t = np.arctan2(y, x)
        return np.hypot(x, y), t + np.where(t < 0.0, two_pi, 0)

    C1, h1 = polar(a1 * scale, b1)
    C2, h2 = polar(a2 * scale, b2)
    lbar = 0.5 * (L1 + L2)
    tmp = (lbar - 50) ** 2
    L_term = (L2 - L1) / (1 + 0.015 * tmp / np.sqrt(20 + tmp))
    cbp = 0.5 * (C1 + C2)
    C_term = (C2 - C1) / (1 + 0.045 * cbp)
    h_diff, h_sum, CC = h2 - h1, h1 + h2, C1 * C2
    if mutant == "nonstrict_pi":
        over, under, wrapped = h_diff >= pi, h_diff <= -pi, np.abs(h_diff) >= pi
    else:
        over, under, wrapped = h_diff > pi, h_diff < -pi, np.abs(h_diff) > pi
    dH = np.where(over, h_diff - two_pi, np.where(under, h_diff + two_pi, h_diff))
    dH = np.where(CC == 0.0, 0.0, dH)
    dH_term = 2 * np.sqrt(CC) * np.sin(dH / 2)
    mask = (CC != 0.0) & wrapped
    low = np.ones_like(mask) if mutant == "hsum_branch" else h_sum < two_pi
    hbar = np.where(mask & low, h_sum + two_pi, np.where(mask & ~low, h_sum - two_pi, h_sum))
    if mutant != "hbar_halved":
        hbar = np.where(CC == 0.0, hbar * 2, hbar)
    hbar = hbar * 0.5
    T = (1 - 0.17 * np.cos(hbar - np.deg2rad(30)) + 0.24 * np.cos(2 * hbar) + 0.32 * np.cos(3 * hbar + np.deg2rad(6))
         - 0.20 * np.cos(4 * hbar - np.deg2rad(63)))
    H_term = dH_term / (1 + 0.015 * cbp * T)
    d7 = cbp ** 7
    Rc = 2 * np.sqrt(d7 / (d7 + p25))
    centre = 270 if mutant == "centre_270" else 275
    dtheta = np.deg2rad(30) * np.exp(-((np.rad2deg(hbar) - centre) / 25) ** 2)
    R_term = -np.sin(2 * dtheta) * Rc * C_term * H_term
    out = np.sqrt(np.maximum(((L_term ** 2 + C_term ** 2) + H_term ** 2) + R_term, 0))
    if parts:
        return out, {"h_diff": h_diff, "h_sum": h_sum, "CC": CC}
    return out


def pair(lab1, lab2, formula=CIEDE2000, mutant=None):
    return cie76(lab1, lab2) if formula == CIE76 else ciede2000(lab1, lab2, mutant)


def crop(img, cb):
    return img if cb == 0 else img[cb:img.shape[0] - cb, cb:img.shape[1] - cb]


def delta_e_map(a, b, formula=CIEDE2000, crop_border=0, mutant=None):
    """The float64 dE of every cropped pixel; byte-equal pairs are exactly 0 (as scikit-image gives them)."""
    a, b = to_rgb(crop(np.asarray(a), crop_border)), to_rgb(crop(np.asarray(b), crop_border))
    d = pair(rgb2lab(a, mutant), rgb2lab(b, mutant), formula, mutant)
    return np.where(np.all(a == b, axis=-1), 0.0, d)


def histogram(dmap):
    idx = np.minimum(np.floor(16.0 * dmap.ravel()), BINS - 1).astype(np.int64)
    return np.bincount(idx, minlength=BINS).astype(np.uint64)


def sums(dmap):
    """The record of a map.  sum and sum2 are math.fsum-exact: the order of additions is not part of the definition."""
    import math
    flat = dmap.ravel()
    return {"count": int(flat.size), "sum": math.fsum(flat.tolist()), "sum2": math.fsum((flat * flat).tolist()),
            "max": float(flat.max()), "hist": histogram(dmap)}


def percentile(hist, count, p):
    """k = max(1, ceil(p count / 100)); the lower edge j / 16 of the first bin whose cumulative count reaches k."""
    k = max(1, -((-Fraction(p) * count) // 100))
    cum = np.cumsum(np.asarray(hist, dtype=object))
    j = next(i for i, c in enumerate(cum) if c >= k)
    return j / 16.0


def fraction_at_least(hist, count, t):
    s = 16.0 * t
    assert s == int(s) and 0 <= s < BINS
    return float(int(np.asarray(hist, dtype=object)[int(s):].sum())) / float(count)


def cells(dmap, x_edges, y_edges):
    """-> (sum, max) arrays, gh x gw, of the map's cells."""
    import math
    gh, gw = len(y_edges) - 1, len(x_edges) - 1
    s, m = np.zeros((gh, gw)), np.zeros((gh, gw))
    for gy in range(gh):
        for gx in range(gw):
            c = dmap[y_edges[gy]:y_edges[gy + 1], x_edges[gx]:x_edges[gx + 1]]
            s[gy, gx] = math.fsum(c.ravel().tolist())
            m[gy, gx] = c.max()
    return s, m


def img_pair(rng, h, w, cn=3, noise=12.0):
    """A smooth colourful image and a noisy, slightly tinted partner, u8; some pixels stay byte-equal."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([128 + 90 * np.sin(xx / 9.0 + 0.3 * c) * np.cos(yy / 7.0 - 0.5 * c) + 30 * np.sin((xx + yy) / 5.0 + c)
                     for c in range(max(cn, 1))], axis=-1)
    a = np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
    keep = rng.random((h, w)) < 0.15
    nb = np.clip(a.astype(np.float64) + rng.normal(0, noise, base.shape) + np.array([4.0, -3.0, 6.0, 0.0][:max(cn, 1)]), 0, 255)
    b = np.where(keep[..., None], a, nb.astype(np.uint8)).astype(np.uint8)
    if cn == 4:
        a[..., 3] = rng.integers(0, 256, (h, w))
        b[..., 3] = rng.integers(0, 256, (h, w))
    if cn == 1:
        a, b = a[..., 0], b[..., 0]
    return np.ascontiguousarray(a), np.ascontiguousarray(b)
