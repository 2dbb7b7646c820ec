"""NumPy / SciPy restatement of the BRISQUE definition in include/sr_hip.h (steps: plane, scale-2 plane, MSCN with a zero
border, products rolled over the whole plane, moments, GGD / AGGD features, scaler and RBF SVR), written from the definition
with library routines -- scipy.ndimage.correlate1d per axis with mode='constant', np.roll on the whole plane,
scipy.special.gamma -- independent of the product.  The luma, the eight taps, the window and the seeded image generator are
_niqe_ref's."""
from __future__ import annotations

import functools
import os

import numpy as np
from scipy import ndimage, special

import _niqe_ref as nref

SHIFTS = nref.SHIFTS                                    # (0, 1), (1, 0), (1, 1), (1, -1)
MOMENTS = nref.MOMENTS
RECORD = np.dtype([("n", "<u8"), ("x", MOMENTS, (5,))])  # sr_brisque_record
GAM = nref.GAM
RINV_GAM = special.gamma(1.0 / GAM) * special.gamma(3.0 / GAM) / special.gamma(2.0 / GAM) ** 2
RINV_MID = (RINV_GAM[1:] + RINV_GAM[:-1]) / 2.0
TILE = 64                                               # the moment kernel's tile side
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "brisque_svr_sklearn.npz")


# ---- steps 1 and 2: the plane and imresize(., 0.5) with ceil sizes --------------------------------------------------------------
def plane(img: np.ndarray, crop_border: int = 0) -> np.ndarray:
    a = np.asarray(img)
    if crop_border:
        a = a[crop_border:a.shape[0] - crop_border, crop_border:a.shape[1] - crop_border]
    y = nref.luma_round(a) if a.ndim == 3 else a.astype(np.int64)
    assert min(y.shape) >= 16
    return y.astype(np.float64)


def _half_axis(p: np.ndarray, axis: int) -> np.ndarray:
    n = p.shape[axis]
    taps = nref.half_taps()
    out = 0.0
    for t in range(8):
        j = 2 * np.arange((n + 1) // 2) - 3 + t
        j = np.where(j < 0, -j - 1, np.where(j >= n, 2 * n - 1 - j, j))
        assert j.min() >= 0 and j.max() < n
        out = out + taps[t] * np.take(p, j, axis=axis)
    return out


def half_plane(p: np.ndarray) -> np.ndarray:
    return _half_axis(_half_axis(p, 1), 0)


# ---- step 3: MSCN, zero border ----------------------------------------------------------------------------------------------
def _blur(a: np.ndarray) -> np.ndarray:
    k = nref.window()
    return ndimage.correlate1d(ndimage.correlate1d(a, k, axis=1, mode="constant", cval=0.0), k, axis=0, mode="constant", cval=0.0)


def mscn(p: np.ndarray) -> np.ndarray:
    mu = _blur(p)
    sigma = np.sqrt(np.abs(_blur(p * p) - mu * mu))
    return (p - mu) / (sigma + 1.0)


# ---- step 4: products over the whole plane, moments -------------------------------------------------------------------------
def _roll_wrap(m, s):
    return np.roll(m, s, axis=(0, 1))


def _roll_pad(m, s, mode):
    """The wrong rolls a wrap probe must tell from the right one: the vacated rim replicates ('edge') or is 0 ('constant')."""
    dy, dx = s
    q = np.pad(m, 1, mode=mode)
    return q[1 - dy:1 - dy + m.shape[0], 1 - dx:1 - dx + m.shape[1]]


def products(m: np.ndarray, roll=_roll_wrap):
    return [m] + [m * roll(m, s) for s in SHIFTS]


def scale_record(p: np.ndarray, roll=_roll_wrap, collect=None) -> np.ndarray:
    rec = np.zeros((), dtype=RECORD)
    rec["n"] = p.size
    for s, x in enumerate(products(mscn(p), roll)):
        if collect is not None:
            collect.append(np.abs(x).min())
        neg, pos = x[x < 0], x[x > 0]
        rec["x"][s] = (neg.size, pos.size, (neg * neg).sum(), (pos * pos).sum(), np.abs(x).sum())
    return rec


def records(img: np.ndarray, crop_border: int = 0, roll=_roll_wrap, collect=None):
    """-> (records[2], 65536 x the half plane as int64)."""
    p = plane(img, crop_border)
    hp = half_plane(p)
    k = hp * 65536.0
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() < 2 ** 25
    return np.stack([scale_record(p, roll, collect), scale_record(hp, roll, collect)]), k.astype(np.int64)


# ---- step 5: features -------------------------------------------------------------------------------------------------------
def ggd(mom, n: float):
    """-> (alpha, s2, rho)."""
    if mom["sabs"] == 0:
        return (np.nan,) * 3
    s2, e = (mom["ssq_neg"] + mom["ssq_pos"]) / n, mom["sabs"] / n
    rho = s2 / e ** 2
    return GAM[int(np.argmin(np.abs(RINV_GAM - rho)))], s2, rho


def aggd(mom, n: float):
    """-> (alpha, mean, ls^2, rs^2, R)."""
    if mom["n_neg"] == 0 or mom["n_pos"] == 0:
        return (np.nan,) * 5
    ls, rs = np.sqrt(mom["ssq_neg"] / float(mom["n_neg"])), np.sqrt(mom["ssq_pos"] / float(mom["n_pos"]))
    g = ls / rs
    rhat = (mom["sabs"] / n) ** 2 / ((mom["ssq_neg"] + mom["ssq_pos"]) / n)
    big_r = rhat * (g ** 3 + 1) * (g + 1) / (g ** 2 + 1) ** 2
    alpha = GAM[int(np.argmin((nref.R_GAM - big_r) ** 2))]
    g1, g2, g3 = (special.gamma(i / alpha) for i in (1.0, 2.0, 3.0))
    return alpha, (rs - ls) * (g2 / g1) * (np.sqrt(g1) / np.sqrt(g3)), ls * ls, rs * rs, big_r


def features(rec: np.ndarray, mids=None) -> np.ndarray:
    """records[2] -> feat[36]; mids: a list that receives every fit's relative distance to the nearest table midpoint."""
    feat = []
    for s in range(2):
        n = float(rec[s]["n"])
        alpha, s2, rho = ggd(rec[s]["x"][0], n)
        feat += [alpha, s2]
        if mids is not None:
            mids.append(np.abs(rho - RINV_MID).min() / rho)
        for i in range(1, 5):
            a, mean, l2, r2, big_r = aggd(rec[s]["x"][i], n)
            feat += [a, mean, l2, r2]
            if mids is not None:
                mids.append(float(nref.midpoint_distance(big_r)[0]))
    return np.array(feat)


ALPHA_SLOTS = nref.alpha_slots()


# ---- step 6: score ----------------------------------------------------------------------------------------------------------
def score(feat, model) -> float:
    f = np.asarray(feat, dtype=np.float64)
    if np.isnan(f).any():
        return float("nan")
    lo, up = model.get("lower", -1.0), model.get("upper", 1.0)
    fmin, fmax = np.asarray(model["feature_min"]).reshape(-1), np.asarray(model["feature_max"]).reshape(-1)
    span = fmax - fmin
    x = np.where(span == 0, 0.0, lo + (up - lo) * (f - fmin) / np.where(span == 0, 1.0, span))
    k = np.exp(-model["gamma"] * ((np.asarray(model["sv"]) - x) ** 2).sum(axis=1))
    return float(np.asarray(model["sv_coef"]).reshape(-1) @ k - model["rho"])


@functools.lru_cache(maxsize=None)
def fixture_model():
    """The committed libsvm (scikit-learn SVR) fit, as it is in tests/golden/brisque_svr_sklearn.npz."""
    with np.load(GOLDEN, allow_pickle=False) as z:
        m = {"sv": z["sv"].copy(), "sv_coef": z["sv_coef"].reshape(-1).copy(), "gamma": float(z["gamma"]),
             "rho": float(z["rho"]), "feature_min": z["feature_min"].copy(), "feature_max": z["feature_max"].copy(),
             "lower": float(z["lower"]), "upper": float(z["upper"])}
    for v in m.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)                     # shared among the tests: read-only
    return m


# ---- shared, cached cases ---------------------------------------------------------------------------------------------------
# (h, w, crop_border): the minimum (one partial tile owns every wrap), one full tile, 2 x 2 tiles with one-pixel and T - 1
# remainders and odd sides, an interior tile, and a crop with an odd byte offset and an odd width
SHAPES = ((16, 16, 0), (TILE, TILE, 0), (TILE + 1, 2 * TILE - 1, 0), (3 * TILE, 3 * TILE, 0), (200, 301, 3))


def case_seed(h: int, w: int, cn: int) -> int:
    return 500000 + 1000 * h + 10 * w + cn


@functools.lru_cache(maxsize=None)
def case(h: int, w: int, cb: int, cn: int):
    """-> (image, records, half plane ints, features, [midpoint distance of every fit], [least |X|]); made once, read-only."""
    img = nref.image(case_seed(h, w, cn), h, w, cn)
    img.setflags(write=False)
    least, mids = [], []
    rec, half = records(img, cb, collect=least)
    feat = features(rec, mids)
    for a in (rec, half, feat):
        a.setflags(write=False)
    return img, rec, half, feat, np.array(mids), np.array(least)


WRAP_SHAPE = (TILE + 1, 2 * TILE - 1, 0, 1)


@functools.lru_cache(maxsize=None)
def wrap_probe():
    """One of the cases' images with its last row and last column overwritten by values far from the first row's (dark,
    alternating) -> (image, records with the right roll, with the replicate roll, with the zero roll)."""
    h, w, cb, cn = WRAP_SHAPE
    img = case(h, w, cb, cn)[0].copy()
    rng = np.random.default_rng(77)
    img[-1, :] = rng.integers(0, 40, size=w)
    img[:, -1] = rng.integers(0, 40, size=h)
    img.setflags(write=False)
    return (img, records(img)[0], records(img, roll=lambda m, s: _roll_pad(m, s, "edge"))[0],
            records(img, roll=lambda m, s: _roll_pad(m, s, "constant"))[0])


def perturbed(rec: np.ndarray, seed: int, rel: float = 1e-9) -> np.ndarray:
    rng = np.random.default_rng(seed)
    out = rec.copy()
    for name in ("ssq_neg", "ssq_pos", "sabs"):
        out["x"][name] *= 1.0 + rel * rng.choice((-1.0, 1.0), size=out["x"][name].shape)
    return out


@functools.lru_cache(maxsize=None)
def score_bar():
    """-> (the largest change of this restatement's score when its moments move by a seeded relative 1e-9, over the cases and
    both channel counts; the bar: 100 x that), as _niqe_ref.score_bar."""
    model = fixture_model()
    worst = 0.0
    for (h, w, cb) in SHAPES:
        for cn in (1, 3):
            rec, feat = case(h, w, cb, cn)[1], case(h, w, cb, cn)[3]
            s0 = score(feat, model)
            for seed in (1, 2, 3):
                worst = max(worst, abs(score(features(perturbed(rec, seed)), model) - s0))
    return worst, 100.0 * worst
