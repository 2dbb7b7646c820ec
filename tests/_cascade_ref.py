"""NumPy restatement of the cascade definition (include/sr_hip.h, "Cascade") in the definition's literal order, the reference
of tests/test_cascade_host.py and tests/test_gpu_cascade.py.  The resize takes its per-axis taps and weights in Python
integers and combines them in int64 (every term stays below 2^35); the tables are int64 cumsum tables that never wrap.  A
second evaluator, ``brute_*``, sums the pixels of every block and rectangle directly, without any table.  ``mut`` names one
deliberate mistake (the mutants of test_cascade_host.py); the default is the definition.

A model here is the dict of tiling_module.load_cascade (or one of the constructed cascades below)."""
import math
import os

import numpy as np

from _mser_ref import baseline_source, gray_swapped  # noqa: F401  (the gray plane of the content section)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LBP_XML = os.path.join(ROOT, "tests", "golden", "lbpcascade_frontalface_opencv.xml")
SKIMAGE_NPZ = os.path.join(ROOT, "tests", "golden", "cascade_skimage.npz")
f32 = np.float32


def rnd(v):
    """Round half to even, in double."""
    return int(round(float(v)))


def scale_list(w, h, model, scale_factor=1.1, min_size=(0, 0), max_size=None, mut=None):
    W0, H0 = model["window"]
    max_w, max_h = max_size if max_size else (w, h)
    out, f = [], 1.0
    while True:
        ww, wh, sw, sh = rnd(W0 * f), rnd(H0 * f), rnd(w / f), rnd(h / f)
        if ww > max_w or wh > max_h or sw < W0 or sh < H0:
            break
        if not (ww < min_size[0] or wh < min_size[1]):
            step = 1 if mut == "step1" else (2 if f <= 2 else 1)
            last_x, last_y = (sw - W0, sh - H0) if mut != "exclusive_last" else (sw - W0 - 1, sh - H0 - 1)
            out.append(dict(f=f, win_w=ww, win_h=wh, sw=sw, sh=sh, step=step,
                            nx=last_x // step + 1 if last_x >= 0 else 0, ny=last_y // step + 1 if last_y >= 0 else 0))
        f = f * scale_factor
    return out


def _axis(n, sn):
    """Per output sample: the two clamped taps and their integer weights over the denominator 2 sn."""
    i0, i1, w0, w1 = [], [], [], []
    for x in range(sn):
        num, den = (2 * x + 1) * n - sn, 2 * sn
        i = num // den
        r = num - i * den
        i0.append(min(max(i, 0), n - 1))
        i1.append(min(max(i + 1, 0), n - 1))
        w0.append(den - r)
        w1.append(r)
    return np.array(i0), np.array(i1), np.array(w0, np.int64), np.array(w1, np.int64)


def resize(g, sw, sh):
    h, w = g.shape
    x0, x1, a0, a1 = _axis(w, sw)
    y0, y1, b0, b1 = _axis(h, sh)
    G = g.astype(np.int64)
    top = G[y0][:, x0] * a0 + G[y0][:, x1] * a1
    bot = G[y1][:, x0] * a0 + G[y1][:, x1] * a1
    D = 4 * sw * sh
    return ((top * b0[:, None] + bot * b1[:, None] + D // 2) // D).astype(np.uint8)


def tables(p):
    T = np.zeros((p.shape[0] + 1, p.shape[1] + 1), np.int64)
    T[1:, 1:] = np.cumsum(np.cumsum(p.astype(np.int64), axis=0), axis=1)
    S = np.zeros_like(T)
    S[1:, 1:] = np.cumsum(np.cumsum(p.astype(np.int64) ** 2, axis=0), axis=1)
    return T, S


def _box(T, x, y, w, h):
    return int(T[y + h, x + w] - T[y, x + w] - T[y + h, x] + T[y, x])


def _brute_box(p, x, y, w, h, square=False):
    blk = p[y:y + h, x:x + w].astype(np.int64)
    return int((blk * blk).sum() if square else blk.sum())


LBP_ORDER = (0, 1, 2, 5, 8, 7, 6, 3)         # bits 7 .. 0


def lbp_code(boxsum, x, y, rect, mut=None):
    fx, fy, bw, bh = rect
    b = [boxsum(x + fx + (k % 3) * bw, y + fy + (k // 3) * bh, bw, bh) for k in range(9)]
    order = LBP_ORDER[1:] + LBP_ORDER[:1] if mut == "bit_order" else LBP_ORDER
    code = 0
    for k in order:
        code = code << 1 | int(b[k] > b[4] if mut == "strict" else b[k] >= b[4])
    return code


class Margins:
    """The smallest relative distance |val - thr nf| / max(|val|, |thr nf|) over the Haar stumps evaluated."""

    def __init__(self):
        self.worst = math.inf

    def see(self, val, lim):
        m = max(abs(val), abs(lim))
        self.worst = min(self.worst, abs(val - lim) / m if m else 0.0)


def window_stages(model, boxsum, boxsq, x, y, mut=None, margins=None):
    """How many stages the window at (x, y) passes before the first it fails."""
    W0, H0 = model["window"]
    haar = model["feature_type"] == "HAAR"
    if haar:
        nr = (0, 0, W0, H0) if mut == "norm_whole" else (1, 1, W0 - 2, H0 - 2)
        A, s, q = nr[2] * nr[3], boxsum(x + nr[0], y + nr[1], nr[2], nr[3]), boxsq(x + nr[0], y + nr[1], nr[2], nr[3])
        v = A * q - s * s
        nf = math.sqrt(float(v)) if v > 0 else 1.0
    k = 0
    for si, (thr, cnt) in enumerate(zip(model["stage_thresholds"], model["stage_counts"])):
        total = f32(0)
        for _ in range(int(cnt)):
            fi = int(model["stump_feature"][k])
            if haar:
                val = None
                for i in range(int(model["feature_nrects"][fi])):
                    rx, ry, rw, rh = (int(v) for v in model["feature_rects"][fi][i])
                    prod = float(model["feature_weights"][fi][i]) * float(boxsum(x + rx, y + ry, rw, rh))
                    val = prod if val is None else val + prod
                lim = float(f32(model["stump_threshold"][k])) * nf
                if margins is not None:
                    margins.see(val, lim)
                first = val < lim
            else:
                code = lbp_code(boxsum, x, y, [int(v) for v in model["feature_rects"][fi]], mut)
                first = bool(int(model["stump_subsets"][k][code >> 5]) & 0xFFFFFFFF & (1 << (code & 31)))
                if mut == "subset_inverted":
                    first = not first
            total = f32(total + f32(model["stump_leaves"][k][0 if first else 1]))
            k += 1
        if (total <= f32(thr)) if mut == "stage_le" else (total < f32(thr)):
            return si
    return len(model["stage_thresholds"])


def stage_map(model, plane, step=1, mut=None, brute=False, margins=None, exclusive=False):
    """int32 [ny, nx]: stages passed per position of one plane."""
    W0, H0 = model["window"]
    sh, sw = plane.shape
    if sw < W0 or sh < H0:
        return np.zeros((0, 0), np.int32)
    if brute:
        boxsum = lambda x, y, w, h: _brute_box(plane, x, y, w, h)                                      # noqa: E731
        boxsq = lambda x, y, w, h: _brute_box(plane, x, y, w, h, True)                                 # noqa: E731
    else:
        T, S = tables(plane)
        boxsum = lambda x, y, w, h: _box(T, x, y, w, h)                                                # noqa: E731
        boxsq = lambda x, y, w, h: _box(S, x, y, w, h)                                                 # noqa: E731
    last_x, last_y = sw - W0 - int(exclusive), sh - H0 - int(exclusive)
    xs, ys = range(0, last_x + 1, step), range(0, last_y + 1, step)
    return np.array([[window_stages(model, boxsum, boxsq, x, y, mut, margins) for x in xs] for y in ys],
                    np.int32).reshape(len(ys), len(xs))


def planes(g, model, **kw):
    return [resize(g, s["sw"], s["sh"]) for s in scale_list(g.shape[1], g.shape[0], model, **kw)]


def candidates(g, model, scale_factor=1.1, min_size=(0, 0), max_size=None, mut=None, brute=False, margins=None):
    """The raw candidates [(x, y, w, h)] in canonical order."""
    out = []
    n_stages = len(model["stage_thresholds"])
    for s in scale_list(g.shape[1], g.shape[0], model, scale_factor, min_size, max_size, mut):
        m = stage_map(model, resize(g, s["sw"], s["sh"]), s["step"], mut, brute, margins, exclusive=mut == "exclusive_last")
        for iy, ix in np.argwhere(m == n_stages):
            x, y = int(ix) * s["step"] * s["f"], int(iy) * s["step"] * s["f"]
            out.append((math.floor(x), math.floor(y), s["win_w"], s["win_h"]) if mut == "floor_candidate"
                       else (rnd(x), rnd(y), s["win_w"], s["win_h"]))
    return out


def _similar(a, b):
    delta = 0.2 * (min(a[2], b[2]) + min(a[3], b[3])) * 0.5
    return (abs(a[0] - b[0]) <= delta and abs(a[1] - b[1]) <= delta and abs(a[0] + a[2] - b[0] - b[2]) <= delta
            and abs(a[1] + a[3] - b[1] - b[3]) <= delta)


def group(cands, min_neighbors=4, mut=None):
    cands = [tuple(int(v) for v in c) for c in cands]
    if min_neighbors == 0:
        return cands
    label = list(range(len(cands)))
    changed = True
    while changed:                               # the transitive closure, the slow and obvious way
        changed = False
        for i in range(len(cands)):
            for j in range(len(cands)):
                if label[i] != label[j] and _similar(cands[i], cands[j]):
                    lo = min(label[i], label[j])
                    label[i] = label[j] = lo
                    changed = True
    classes = []
    for first in sorted(set(label)):
        mem = [c for c, l in zip(cands, label) if l == first]
        s = f32(1) / f32(len(mem))
        classes.append((tuple(int(np.rint(f32(f32(sum(m[k] for m in mem)) * s))) for k in range(4)), len(mem)))
    out = []
    for i, (r1, n1) in enumerate(classes):
        if (n1 < min_neighbors) if mut == "n_lt" else (n1 <= min_neighbors):
            continue
        for j, (r2, n2) in enumerate(classes):
            if j == i or n2 <= min_neighbors:
                continue
            dx, dy = rnd(r2[2] * 0.2), rnd(r2[3] * 0.2)
            if (r1[0] >= r2[0] - dx and r1[1] >= r2[1] - dy and r1[0] + r1[2] <= r2[0] + r2[2] + dx
                    and r1[1] + r1[3] <= r2[1] + r2[3] + dy and (n2 > max(3, n1) or n1 < 3)):
                break
        else:
            out.append(r1)
    return out


# ---- models ---------------------------------------------------------------------------------------------------------------
def _lbp(window, stages, feats):
    """stages: [(threshold, [(feature, subsets[8], leaf0, leaf1)])]"""
    stumps = [s for _, st in stages for s in st]
    return {"feature_type": "LBP", "window": window,
            "stage_thresholds": np.array([t for t, _ in stages], f32), "stage_counts": np.array([len(st) for _, st in stages], np.int32),
            "stump_feature": np.array([s[0] for s in stumps], np.int32),
            "stump_subsets": np.array([s[1] for s in stumps], np.uint32).view(np.int32).reshape(-1, 8),
            "stump_leaves": np.array([[s[2], s[3]] for s in stumps], f32).reshape(-1, 2),
            "feature_rects": np.array(feats, np.int32).reshape(-1, 4)}


def accept_all(window=(24, 24)):
    return _lbp(window, [(-1.0, [])], [])


def reject_all(window=(24, 24)):
    return _lbp(window, [(1.0, [])], [])


def random_lbp_stumps(rng, window, n, n_feats=12):
    feats = []
    for _ in range(n_feats):
        bw, bh = int(rng.integers(1, window[0] // 3 + 1)), int(rng.integers(1, window[1] // 3 + 1))
        feats.append((int(rng.integers(0, window[0] - 3 * bw + 1)), int(rng.integers(0, window[1] - 3 * bh + 1)), bw, bh))
    stumps = [(int(rng.integers(0, n_feats)), [int(v) for v in rng.integers(0, 2 ** 32, size=8)],
               float(f32(rng.uniform(-1, 1))), float(f32(rng.uniform(-1, 1)))) for _ in range(n)]
    return feats, stumps


def checker(window=(24, 24), seed=3, tail=70):
    """Stage 0: one stump on the 3 x 3 pixels at the window's corner that passes exactly the windows whose centre pixel
    (1, 1) is not above any of its eight neighbours (code 255): on ``checker_image`` a checkerboard half of the step-2
    positions of scale 0.  Stage 1: ``tail`` random stumps, more than the dense stages hold, so the survivors are compacted
    right after stage 0."""
    rng = np.random.default_rng(seed)
    feats, stumps = random_lbp_stumps(rng, window, tail)
    only255 = [0] * 7 + [1 << 31]
    return _lbp(window, [(0.0, [(len(feats), only255, 1.0, -1.0)]), (0.0, stumps)], feats + [(0, 0, 1, 1)])


def permissive_then_tail(window=(24, 24), seed=4, tail=65):
    """Stage 0 holds no stump and passes every window; stage 1 holds ``tail`` random stumps, one more than the dense stages
    take: every position reaches the tail kernel."""
    feats, stumps = random_lbp_stumps(np.random.default_rng(seed), window, tail)
    return _lbp(window, [(-1.0, []), (float(f32(0.9 * math.sqrt(tail))), stumps)], feats)


def checker_image(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((xx >> 1) + (yy >> 1)) & 1) * 255).astype(np.uint8)


def random_lbp(window=(24, 24), seed=5, stages=(3, 5, 9, 70, 11)):
    """A random LBP cascade whose thresholds sit low enough that windows reach every stage."""
    rng = np.random.default_rng(seed)
    feats, stumps = random_lbp_stumps(rng, window, sum(stages))
    out, k = [], 0
    for n in stages:
        out.append((float(f32(-0.35 * math.sqrt(n))), stumps[k:k + n]))
        k += n
    return _lbp(window, out, feats)


def random_haar(window=(20, 16), seed=11, stages=(4, 6, 70, 8), n_feats=24):
    """A constructed HAAR cascade: 2- and 3-rectangle features, an outer rectangle of weight -1 and one or two rectangles
    inside it whose weights balance it (outer area over inner area: integers such as 2 and 3 where the areas divide,
    non-integers such as 2.6666667 where they do not), as trained cascades have them."""
    rng = np.random.default_rng(seed)
    W0, H0 = window
    rects, weights, nrects = np.zeros((n_feats, 3, 4), np.int32), np.zeros((n_feats, 3), f32), []
    for i in range(n_feats):
        n = 2 + i % 2
        nrects.append(n)
        ow, oh = int(rng.integers(3, W0 + 1)), int(rng.integers(3, H0 + 1))
        ow -= ow % 2 if i % 3 == 0 else 0        # every third feature: halves of an even width, weights 2 or 1
        ox, oy = int(rng.integers(0, W0 - ow + 1)), int(rng.integers(0, H0 - oh + 1))
        rects[i, 0], weights[i, 0] = (ox, oy, ow, oh), -1.0
        for j in range(1, n):
            rw, rh = (ow // 2, oh) if i % 3 == 0 else (int(rng.integers(1, ow)), int(rng.integers(1, oh)))
            rects[i, j] = (ox + int(rng.integers(0, ow - rw + 1)), oy + int(rng.integers(0, oh - rh + 1)), rw, rh)
            weights[i, j] = f32(ow * oh) / f32((n - 1) * rw * rh)
    ns = sum(stages)
    return {"feature_type": "HAAR", "window": window, "max_rects": 3,
            "stage_thresholds": np.array([-0.35 * math.sqrt(n) for n in stages], f32), "stage_counts": np.array(stages, np.int32),
            "stump_feature": rng.integers(0, n_feats, size=ns).astype(np.int32),
            "stump_threshold": rng.uniform(-0.01, 0.01, size=ns).astype(f32),
            "stump_leaves": rng.uniform(-1, 1, size=(ns, 2)).astype(f32),
            "feature_nrects": np.array(nrects, np.int32), "feature_rects": rects, "feature_weights": weights}


def haar_image(h, w, seed=2):
    """Smooth structure plus noise, with a flat patch larger than a window (the nf = 1 branch)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = 128 + 60 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + rng.normal(0, 12, size=(h, w))
    img[2:2 + min(h - 2, 30), 3:3 + min(w - 3, 36)] = 77
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def noise_image(h, w, seed=1):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(np.rint(120 + 50 * np.sin(xx / 9.0 + yy / 13.0) + rng.normal(0, 25, size=(h, w))), 0, 255).astype(np.uint8)


def skimage_fixture():
    z = np.load(SKIMAGE_NPZ)
    return {k: z[k] for k in z.files}


# The constructed Haar inputs of both test files: name -> (model, image, detection arguments).  The seeds are chosen so that
# the restatement keeps every stump's |val - thr nf| well away from zero (tests/test_cascade_host.py asserts it).
HAAR_INPUTS = {
    "noise": lambda: (random_haar(), noise_image(40, 47, 6), {}),
    "flat": lambda: (random_haar(seed=12), haar_image(44, 52), {}),
    "wide_window": lambda: (random_haar(window=(31, 12), seed=13), haar_image(30, 70, 3), dict(scale_factor=1.25)),
}
