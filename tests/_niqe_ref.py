"""NumPy / SciPy restatement of the NIQE definition in include/sr_hip.h (steps: plane, scale-2 plane, MSCN, block moments,
AGGD features, score, fit), written from the definition with library routines -- scipy.ndimage.correlate1d per axis with
mode='nearest', np.roll on each block, scipy.special.gamma, np.linalg.pinv, np.cov -- and a seeded image generator whose
images keep every MSCN value and product away from 0 and every fit away from a midpoint of the Gamma-ratio table (the guards
are tests/test_niqe_host.py's)."""
from __future__ import annotations

import functools

import numpy as np
from scipy import ndimage, special

BLOCK = 96
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
MOMENTS = np.dtype([("n_neg", "<u8"), ("n_pos", "<u8"), ("ssq_neg", "<f8"), ("ssq_pos", "<f8"), ("sabs", "<f8")])
RECORD = np.dtype([("x", MOMENTS, (5,)), ("sum_sigma", "<f8")])          # sr_niqe_block
GAM = 0.2 + 0.001 * np.arange(9801)
R_GAM = special.gamma(2.0 / GAM) ** 2 / (special.gamma(1.0 / GAM) * special.gamma(3.0 / GAM))
R_MID = (R_GAM[1:] + R_GAM[:-1]) / 2.0


# ---- images -----------------------------------------------------------------------------------------------------------------
def image(seed: int, h: int, w: int, cn: int = 1, field_amp: float = 40.0, noise: float = 12.0) -> np.ndarray:
    """A 4 x 4-pixel-blocky Gaussian field x 40 plus Gaussian noise of sigma 12 around 128, rounded and clipped (cn = 3: one
    field, the noise of each channel its own)."""
    rng = np.random.default_rng(seed)
    field = np.kron(rng.standard_normal(((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4)))[:h, :w]
    planes = [np.clip(np.rint(128.0 + field_amp * field + noise * rng.standard_normal((h, w))), 0, 255).astype(np.uint8)
              for _ in range(cn)]
    out = planes[0] if cn == 1 else np.stack(planes, -1)
    return np.ascontiguousarray(out)


# ---- step 1: the plane ------------------------------------------------------------------------------------------------------
def luma_round(rgb: np.ndarray) -> np.ndarray:
    v = rgb.astype(np.int64)
    x = 65481 * v[..., 0] + 128553 * v[..., 1] + 24966 * v[..., 2] + 4080000
    return (2 * x + 255000) // 510000


def plane(img: np.ndarray, crop_border: int = 0) -> np.ndarray:
    """-> the kept H x W plane as float64 gray levels (integers)."""
    a = np.asarray(img)
    if crop_border:
        a = a[crop_border:a.shape[0] - crop_border, crop_border:a.shape[1] - crop_border]
    y = luma_round(a) if a.ndim == 3 else a.astype(np.int64)
    nby, nbx = y.shape[0] // BLOCK, y.shape[1] // BLOCK
    assert nby >= 1 and nbx >= 1
    return y[:nby * BLOCK, :nbx * BLOCK].astype(np.float64)


# ---- step 2: imresize(., 0.5) -----------------------------------------------------------------------------------------------
def cubic(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(x <= 1, 1.5 * x ** 3 - 2.5 * x ** 2 + 1, np.where(x <= 2, -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2, 0.0))


def half_taps() -> np.ndarray:
    """The eight taps of every output at scale 1/2: 0.5 cubic(0.5 d), d = the distances 3.5, 2.5, .., -3.5 of inputs 2 i - 3 ..
    2 i + 4 from the output's centre 2 i + 0.5."""
    d = np.arange(-3, 5) - 0.5
    return 0.5 * cubic(0.5 * d)


def _half_axis(p: np.ndarray, axis: int) -> np.ndarray:
    n = p.shape[axis]
    taps = half_taps()
    out = 0.0
    for t in range(8):
        j = 2 * np.arange(n // 2) - 3 + t
        j = np.where(j < 0, -j - 1, np.where(j >= n, 2 * n - 1 - j, j))
        out = out + taps[t] * np.take(p, j, axis=axis)
    return out


def half_plane(p: np.ndarray) -> np.ndarray:
    """Rows first (the pass along each row), then columns; float64 gray levels."""
    return _half_axis(_half_axis(p, 1), 0)


# ---- step 3: MSCN -----------------------------------------------------------------------------------------------------------
def window() -> np.ndarray:
    i = np.arange(-3, 4, dtype=np.float64)
    g = np.exp(-i * i / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


def _blur(a: np.ndarray) -> np.ndarray:
    k = window()
    return ndimage.correlate1d(ndimage.correlate1d(a, k, axis=1, mode="nearest"), k, axis=0, mode="nearest")


def mscn(p: np.ndarray):
    mu = _blur(p)
    sigma = np.sqrt(np.abs(_blur(p * p) - mu * mu))
    return (p - mu) / (sigma + 1.0), sigma


# ---- step 4: blocks and moments ---------------------------------------------------------------------------------------------
def block_products(b: np.ndarray):
    """X_0 .. X_4 of one block."""
    return [b] + [b * np.roll(b, s, axis=(0, 1)) for s in SHIFTS]


def scale_records(p: np.ndarray, side: int, collect=None) -> np.ndarray:
    m, sigma = mscn(p)
    nby, nbx = p.shape[0] // side, p.shape[1] // side
    rec = np.zeros(nby * nbx, dtype=RECORD)
    for by in range(nby):
        for bx in range(nbx):
            sl = (slice(by * side, (by + 1) * side), slice(bx * side, (bx + 1) * side))
            r = rec[by * nbx + bx]
            r["sum_sigma"] = sigma[sl].sum()
            for s, x in enumerate(block_products(m[sl])):
                if collect is not None:
                    collect.append(np.abs(x).min())
                neg, pos = x[x < 0], x[x > 0]
                r["x"][s] = (neg.size, pos.size, (neg * neg).sum(), (pos * pos).sum(), np.abs(x).sum())
    return rec


def records(img: np.ndarray, crop_border: int = 0, collect=None):
    """-> (records[2, nblocks] scale-major, 65536 x the half plane as int64, (H, W, nby, nbx)); collect: a list that receives
    the least |X| of every block, scale and X."""
    p = plane(img, crop_border)
    hp = half_plane(p)
    k = hp * 65536.0
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() < 2 ** 25
    rec = np.stack([scale_records(p, BLOCK, collect), scale_records(hp, BLOCK // 2, collect)])
    return rec, k.astype(np.int64), (p.shape[0], p.shape[1], p.shape[0] // BLOCK, p.shape[1] // BLOCK)


# ---- step 5: features -------------------------------------------------------------------------------------------------------
def aggd(mom, n: float):
    """-> (alpha, beta_l, beta_r, R) of one moments record."""
    if mom["n_neg"] == 0 or mom["n_pos"] == 0:
        return (np.nan,) * 4
    ls, rs = np.sqrt(mom["ssq_neg"] / float(mom["n_neg"])), np.sqrt(mom["ssq_pos"] / float(mom["n_pos"]))
    g = ls / rs
    rhat = (mom["sabs"] / n) ** 2 / ((mom["ssq_neg"] + mom["ssq_pos"]) / n)
    big_r = rhat * (g ** 3 + 1) * (g + 1) / (g ** 2 + 1) ** 2
    alpha = GAM[int(np.argmin((R_GAM - big_r) ** 2))]
    s = np.sqrt(special.gamma(1.0 / alpha) / special.gamma(3.0 / alpha))
    return alpha, ls * s, rs * s, big_r


def features(rec: np.ndarray, fits=None) -> np.ndarray:
    """records[2, nblocks] -> feat[nblocks, 36]; fits: a list that receives the R of every fit."""
    nblocks = rec.shape[1]
    feat = np.zeros((nblocks, 36))
    for s in range(2):
        n = float((BLOCK >> s) ** 2)
        for b in range(nblocks):
            row = []
            for i in range(5):
                alpha, bl, br, big_r = aggd(rec[s, b]["x"][i], n)
                if fits is not None:
                    fits.append(big_r)
                if i == 0:
                    row += [alpha, (bl + br) / 2.0]
                else:
                    row += [alpha, (br - bl) * (special.gamma(2.0 / alpha) / special.gamma(1.0 / alpha)), bl, br]
            feat[b, 18 * s:18 * s + 18] = row
    return feat


def alpha_slots() -> np.ndarray:
    """Which of the 36 features are alphas."""
    one = [0] + [2 + 4 * i for i in range(4)]
    return np.array(one + [18 + i for i in one])


def midpoint_distance(big_r) -> np.ndarray:
    """Relative distance of each R to the nearest midpoint of the Gamma-ratio table."""
    big_r = np.atleast_1d(np.asarray(big_r, dtype=np.float64))
    return np.abs(big_r[:, None] - R_MID[None, :]).min(axis=1) / big_r


def sharpness(rec: np.ndarray) -> np.ndarray:
    return rec[0]["sum_sigma"] / float(BLOCK * BLOCK)


# ---- steps 6 and 7: score and fit -------------------------------------------------------------------------------------------
def score(feat: np.ndarray, mu_pris: np.ndarray, cov_pris: np.ndarray) -> float:
    ok = ~np.isnan(feat).any(axis=1)
    if ok.sum() < 2:
        return float("nan")
    mu_d = np.nanmean(feat, axis=0)
    cov_d = np.cov(feat[ok], rowvar=False)
    d = np.asarray(mu_pris).reshape(-1) - mu_d
    return float(np.sqrt(d @ np.linalg.pinv((np.asarray(cov_pris) + cov_d) / 2.0) @ d))


def fit_rows(feats, sharps, threshold: float = 0.75) -> np.ndarray:
    rows = []
    for f, s in zip(feats, sharps):
        keep = (s > threshold * s.max()) & ~np.isnan(f).any(axis=1)
        rows.append(f[keep])
    return np.concatenate(rows)


def fit(feats, sharps, threshold: float = 0.75):
    rows = fit_rows(feats, sharps, threshold)
    if rows.shape[0] < 37:
        raise ValueError(f"{rows.shape[0]} rows")
    return rows.mean(axis=0), np.cov(rows, rowvar=False), rows.shape[0]


# ---- shared, cached cases ---------------------------------------------------------------------------------------------------
# (h, w, crop_border) of the device tests: one block (every border of both passes in it), the smallest scoreable shape, an
# interior block, and a crop with an odd byte offset and unused margins
SHAPES = ((96, 96, 0), (96, 192, 0), (288, 288, 0), (200, 301, 3))
FIT_SEEDS = (7001, 7002, 7003)
FIT_SHAPE = (480, 576)                      # 30 blocks each


def case_seed(h: int, w: int, cn: int) -> int:
    return 300000 + 1000 * h + 10 * w + cn


@functools.lru_cache(maxsize=None)
def case(h: int, w: int, cb: int, cn: int):
    """-> (image, records, half plane ints, info, features, [R of every fit], [least |X|]); made once, never modified."""
    img = image(case_seed(h, w, cn), h, w, cn)
    img.setflags(write=False)
    least, fits = [], []
    rec, half, info = records(img, cb, least)
    feat = features(rec, fits)
    for a in (rec, half, feat):
        a.setflags(write=False)
    return img, rec, half, info, feat, np.array(fits), np.array(least)


@functools.lru_cache(maxsize=None)
def pristine():
    """The model fitted by this restatement from three other seeded images -> (mu, cov, rows used, feats, sharps)."""
    feats, sharps = [], []
    for seed in FIT_SEEDS:
        rec, _, _ = records(image(seed, *FIT_SHAPE, 1))
        feats.append(features(rec))
        sharps.append(sharpness(rec))
    mu, cov, n = fit(feats, sharps)
    return mu, cov, n, feats, sharps


def perturbed(rec: np.ndarray, seed: int, rel: float = 1e-9) -> np.ndarray:
    """The records with every float sum moved by rel, the sign seeded."""
    rng = np.random.default_rng(seed)
    out = rec.copy()
    for name in ("ssq_neg", "ssq_pos", "sabs"):
        out["x"][name] *= 1.0 + rel * rng.choice((-1.0, 1.0), size=out["x"][name].shape)
    return out


@functools.lru_cache(maxsize=None)
def score_bar():
    """-> (the largest change of this restatement's score when its moments move by a seeded relative 1e-9, over the scoreable
    cases and both channel counts; the bar: 100 x that -- ten for the distance between two correct eigen-solvers, ten for
    headroom)."""
    mu, cov = pristine()[:2]
    worst = 0.0
    for (h, w, cb) in SHAPES[1:]:
        for cn in (1, 3):
            rec, feat = case(h, w, cb, cn)[1], case(h, w, cb, cn)[4]
            s0 = score(feat, mu, cov)
            for seed in (1, 2, 3):
                worst = max(worst, abs(score(features(perturbed(rec, seed)), mu, cov) - s0))
    return worst, 100.0 * worst
