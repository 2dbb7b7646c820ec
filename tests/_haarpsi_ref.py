"""NumPy / SciPy restatement of HaarPSI (Reisenhofer, Bosse, Kutyniok, Wiegand 2018) in the float form of the authors'
scripts: every filter is a dense 2-D convolution of float64 planes.  It shares no code with the library.

convention 'python': scipy.signal.convolve2d(., k, mode='same'), the call the authors' Python script makes.
convention 'matlab': conv2(., k, 'same'), restated as the full convolution cropped at floor(k / 2).
Samples outside a plane are zero in both.  The definition is in include/sr_hip.h.

`mutant` names one deliberate departure from the definition (tests/test_haarpsi_host.py checks that each one moves the
value): 'weight_scale2', 'no_half', 'chroma_max', 'pool_phase', 'replicate', 'alpha', 'C'."""
from __future__ import annotations

import numpy as np
from scipy.signal import convolve2d

C_DEFAULT, ALPHA_DEFAULT, SCALES = 30.0, 4.2, 3
MUTANTS = ("weight_scale2", "no_half", "chroma_max", "pool_phase", "replicate", "alpha", "C")


def conv_same(x: np.ndarray, k: np.ndarray, convention: str, replicate: bool = False) -> np.ndarray:
    """The 'same' convolution of the plane x with the kernel k under `convention`."""
    if convention not in ("matlab", "python"):
        raise ValueError(convention)
    if replicate:                   # (mutant) the border replicates instead of being zero
        py, px = k.shape[0], k.shape[1]
        xp = np.pad(x, ((py, py), (px, px)), mode="edge")
        return conv_same(xp, k, convention)[py:-py, px:-px]
    if convention == "python":
        return convolve2d(x, k, mode="same")
    full = convolve2d(x, k, mode="full")
    r0, c0 = k.shape[0] // 2, k.shape[1] // 2
    return full[r0:r0 + x.shape[0], c0:c0 + x.shape[1]]


def planes(img: np.ndarray):
    """Y, I, Q (float64) of a u8 image: gray (H x W or one channel), RGB or RGBA (alpha ignored)."""
    a = np.asarray(img).astype(np.float64)
    if a.ndim == 2 or a.shape[2] == 1:
        return a.reshape(a.shape[0], a.shape[1]), None, None
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    return 0.299 * r + 0.587 * g + 0.114 * b, 0.596 * r - 0.274 * g - 0.322 * b, 0.211 * r - 0.523 * g + 0.312 * b


def haar_kernel(scale: int) -> np.ndarray:
    n = 2 ** scale
    k = np.full((n, n), 2.0 ** -scale)
    k[: n // 2, :] *= -1.0
    return k


def haarpsi_ref(ref: np.ndarray, dist: np.ndarray, crop_border: int = 0, subsample: bool = True, convention: str = "matlab",
                mutant: str | None = None) -> dict:
    """-> {'num': [channels], 'den': [channels], 'value', 'map_num', 'map_den' (per sample, summed over channels)}."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(mutant)
    ref, dist = np.asarray(ref), np.asarray(dist)
    if ref.shape != dist.shape:
        raise ValueError("shapes differ")
    cb = int(crop_border)
    if cb:
        ref, dist = ref[cb:ref.shape[0] - cb, cb:ref.shape[1] - cb], dist[cb:dist.shape[0] - cb, cb:dist.shape[1] - cb]
    C = 40.0 if mutant == "C" else C_DEFAULT
    alpha = 4.5 if mutant == "alpha" else ALPHA_DEFAULT
    rep = mutant == "replicate"
    pool_conv = convention if mutant != "pool_phase" else ("python" if convention == "matlab" else "matlab")
    pa, pb = list(planes(ref)), list(planes(dist))
    colour = pa[1] is not None
    if subsample:
        box = np.full((2, 2), 0.25)
        pa = [None if p is None else conv_same(p, box, pool_conv, rep)[::2, ::2] for p in pa]
        pb = [None if p is None else conv_same(p, box, pool_conv, rep)[::2, ::2] for p in pb]

    def coeffs(y):
        out = []
        for k in (haar_kernel(s) for s in range(1, SCALES + 1)):
            out.append((np.abs(conv_same(y, k, convention, rep)), np.abs(conv_same(y, k.T, convention, rep))))
        return out          # [scale][orientation]

    ca, cb_ = coeffs(pa[0]), coeffs(pb[0])

    def sim(a, b):
        return (2.0 * a * b + C) / (a * a + b * b + C)

    wscale = 1 if mutant == "weight_scale2" else 2
    half = 1.0 if mutant == "no_half" else 0.5
    ls, wt = [], []
    for d in range(2):
        wt.append(np.maximum(ca[wscale][d], cb_[wscale][d]))
        ls.append(half * (sim(ca[0][d], cb_[0][d]) + sim(ca[1][d], cb_[1][d])))
    if colour:
        box = np.full((2, 2), 0.25)
        ci = [np.abs(conv_same(p[1], box, convention, rep)) for p in (pa, pb)]
        cq = [np.abs(conv_same(p[2], box, convention, rep)) for p in (pa, pb)]
        ls.append(0.5 * (sim(ci[0], ci[1]) + sim(cq[0], cq[1])))
        wt.append(np.maximum(wt[0], wt[1]) if mutant == "chroma_max" else 0.5 * (wt[0] + wt[1]))
    sig = [1.0 / (1.0 + np.exp(-alpha * l)) for l in ls]
    num = np.array([float(np.sum(s * w)) for s, w in zip(sig, wt)])
    den = np.array([float(np.sum(w)) for w in wt])
    with np.errstate(invalid="ignore", divide="ignore"):
        x = num.sum() / den.sum() if den.sum() != 0.0 else float("nan")
        value = (np.log(x / (1.0 - x)) / alpha) ** 2
    return {"num": num, "den": den, "value": float(value), "channels": len(wt),
            "map_num": sum(s * w for s, w in zip(sig, wt)), "map_den": sum(wt)}


def anchor_pair(h: int = 17, w: int = 33):
    """The cross-check input of the definition: a[y, x, k] = (7 y + 13 x + 31 k + 5 ((y x) mod 11)) mod 256 and
    b = clip(a + 3 ((y x + k) mod 9) - 12, 0, 255)."""
    y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    a = (7 * y + 13 * x + 31 * k + 5 * ((y * x) % 11)) % 256
    b = np.clip(a + 3 * ((y * x + k) % 9) - 12, 0, 255)
    return a.astype(np.uint8), b.astype(np.uint8)


ANCHORS = {      # (colour, convention, subsample) -> value
    (True, "matlab", True): 0.9823113909793684, (True, "python", True): 0.9763492583186448,
    (True, "matlab", False): 0.9002864697615205, (True, "python", False): 0.9016563738562563,
    (False, "matlab", True): 0.981379568642581, (False, "python", True): 0.969539076338017,
    (False, "matlab", False): 0.8552551966335398, (False, "python", False): 0.850741129315345,
}
ANCHOR_NUM = (36361.7884372, 32570.3405328, 34488.2535139)      # RGB, 'matlab', subsampled
ANCHOR_DEN = (36936.242625, 33083.88325, 35010.0629375)
