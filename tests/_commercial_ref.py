"""NumPy restatement of the reference's commercial / no-reference metrics (quality_assessment_module.py:611-1193) with
every cv2 call pinned to one written-out rule.  Rules marked † restate OpenCV 4.x from memory (no cv2 on the build
machines): they define what the HIP kernels compute and cannot be checked against OpenCV itself here.

  gray          cv2.COLOR_RGB2GRAY, fixed point 15 (OpenCV >= 4) or 14 bits
  reflect-101   np.pad(mode="reflect") -- cv2.BORDER_REFLECT_101 including the repeated reflection of tiny images
  Laplacian     ksize 1: [0 1 0; 1 -4 1; 0 1 0], exact
  GaussianBlur  3x3, sigma 0: [1/4 1/2 1/4] (exact on integers)
  MSCN †        7x7, sigma 7/6: weights exp(-(i-3)^2 / (2 sigma^2)) normalised in fp64, rounded to float32; row pass then
                column pass, taps left to right / top to bottom, acc = acc + w * v in float32 without contraction
  blur 5x5 †    float32(S * (1/25)) from the exact integer box sum S (boxFilter's double sums)
  Sobel         3x3, exact; reflect-101 (BRISQUE) or replicate (Canny, CV_16S)
  Canny †       L1 magnitude, TG22 = 13573 sectors, NMS with 0 outside the image, candidates m > 50, strong m > 150, edges =
                candidates 8-connected through candidates to a strong pixel
  Lab †         8-bit RGB2Lab: sRGB gamma table x 2^3, D65 coefficients x 2^12, cube-root table x 2^15 (3072 entries),
                L = descale(296 fY + Lshift, 15), a/b = descale(500 (fX - fY) / 200 (fY - fZ) + 128 << 15, 15), saturated
  YCrCb †       Y = descale(4899 R + 9617 G + 1868 B, 14), Cr = descale((R - Y) 11682 + 128 << 14, 14), Cb with B and 9241
"""
from __future__ import annotations

import numpy as np

# ---- elementary rules --------------------------------------------------------------------------------------------------


def gray_of(img: np.ndarray, shift: int = 15) -> np.ndarray:
    if img.ndim == 2:
        return img.astype(np.int64)
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    if shift == 15:
        return (r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15
    return (r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14


def pad101(a: np.ndarray, p: int) -> np.ndarray:
    # axis by axis: a length-1 axis repeats its value (borderInterpolate's answer), any other reflects
    for ax in range(a.ndim):
        width = [(0, 0)] * a.ndim
        width[ax] = (p, p)
        a = np.pad(a, width, mode="reflect" if a.shape[ax] > 1 else "edge")
    return a


def shifted(P: np.ndarray, p: int, dy: int, dx: int, h: int, w: int) -> np.ndarray:
    return P[p + dy:p + dy + h, p + dx:p + dx + w]


def gauss7_weights() -> np.ndarray:
    """† cv2.getGaussianKernel(7, 7/6, CV_32F)."""
    s = 7.0 / 6.0
    w = np.exp(-((np.arange(7) - 3.0) ** 2) / (2.0 * s * s))
    return (w / w.sum()).astype(np.float32)


def laplacian(g: np.ndarray) -> np.ndarray:
    h, w = g.shape
    P = pad101(g, 1)
    return (shifted(P, 1, -1, 0, h, w) + shifted(P, 1, 1, 0, h, w) + shifted(P, 1, 0, -1, h, w) +
            shifted(P, 1, 0, 1, h, w) - 4 * g)


def noise16(g: np.ndarray) -> np.ndarray:
    """16 (g - GaussianBlur(g, 3x3, 0)): an exact integer."""
    h, w = g.shape
    P = pad101(g, 1)
    k = (1, 2, 1)
    b = sum(k[i] * k[j] * shifted(P, 1, i - 1, j - 1, h, w) for i in range(3) for j in range(3))
    return 16 * g - b


def sobel(g: np.ndarray, replicate: bool = False):
    h, w = g.shape
    P = np.pad(g, 1, mode="edge") if replicate else pad101(g, 1)
    a = {(i, j): shifted(P, 1, i, j, h, w) for i in (-1, 0, 1) for j in (-1, 0, 1)}
    gx = (a[-1, 1] - a[-1, -1]) + 2 * (a[0, 1] - a[0, -1]) + (a[1, 1] - a[1, -1])
    gy = (a[1, -1] - a[-1, -1]) + 2 * (a[1, 0] - a[-1, 0]) + (a[1, 1] - a[-1, 1])
    return gx, gy


def local_variance5(g: np.ndarray) -> np.ndarray:
    """† blur(g^2, 5x5) - blur(g, 5x5)^2 in float32."""
    h, w = g.shape
    P = pad101(g, 2)
    s = sum(shifted(P, 2, i, j, h, w) for i in range(-2, 3) for j in range(-2, 3))
    s2 = sum(shifted(P, 2, i, j, h, w) ** 2 for i in range(-2, 3) for j in range(-2, 3))
    bm = (s.astype(np.float64) * (1.0 / 25.0)).astype(np.float32)
    bq = (s2.astype(np.float64) * (1.0 / 25.0)).astype(np.float32)
    return bq - bm * bm


def mscn(g: np.ndarray) -> np.ndarray:
    """† the float32 MSCN map of _calculate_niqe_simple / _calculate_brisque_simple in the stated order."""
    h, w = g.shape
    wt = gauss7_weights()
    P = pad101(g, 3).astype(np.float32)
    P2 = P * P
    ra = np.zeros((h + 6, w), np.float32)
    rb = np.zeros((h + 6, w), np.float32)
    for j in range(7):
        ra = ra + wt[j] * P[:, j:j + w]
        rb = rb + wt[j] * P2[:, j:j + w]
    mu = np.zeros((h, w), np.float32)
    e2 = np.zeros((h, w), np.float32)
    for i in range(7):
        mu = mu + wt[i] * ra[i:i + h]
        e2 = e2 + wt[i] * rb[i:i + h]
    sigma = np.sqrt(np.maximum(e2 - mu * mu, np.float32(0)))
    return (g.astype(np.float32) - mu) / (sigma + np.float32(1.0))


# ---- Canny -------------------------------------------------------------------------------------------------------------
TG22 = 13573


def canny_nms(g: np.ndarray, low: int = 50, high: int = 150) -> np.ndarray:
    """† state map: 0 none, 1 candidate (survives NMS, m > low), 2 strong (candidate with m > high)."""
    h, w = g.shape
    dx, dy = sobel(g, replicate=True)
    m = np.abs(dx) + np.abs(dy)
    M = np.pad(m, 1)                                  # magnitudes outside the image are 0
    at = lambda oy, ox: M[1 + oy:1 + oy + h, 1 + ox:1 + ox + w]
    ax, ay = np.abs(dx), np.abs(dy) << 15
    tg22x = ax * TG22
    tg67x = tg22x + (ax << 16)
    horiz = ay < tg22x
    vert = ~horiz & (ay > tg67x)
    diag = ~horiz & ~vert
    s = np.where((dx ^ dy) < 0, -1, 1)
    keep_h = (m > at(0, -1)) & (m >= at(0, 1))
    keep_v = (m > at(-1, 0)) & (m >= at(1, 0))
    up_m = np.where(s < 0, at(-1, 1), at(-1, -1))     # up[x - s]
    dn_p = np.where(s < 0, at(1, -1), at(1, 1))       # down[x + s]
    keep_d = (m > up_m) & (m > dn_p)
    keep = (m > low) & ((horiz & keep_h) | (vert & keep_v) | (diag & keep_d))
    st = np.zeros((h, w), np.uint8)
    st[keep] = 1
    st[keep & (m > high)] = 2
    return st


def canny_edges(g: np.ndarray, low: int = 50, high: int = 150) -> np.ndarray:
    """Edge set as components: every candidate 8-connected through candidates to a strong pixel (scipy labelling)."""
    from scipy import ndimage
    st = canny_nms(g, low, high)
    lab, n = ndimage.label(st > 0, structure=np.ones((3, 3), bool))
    strong_labels = np.unique(lab[st == 2])
    return np.isin(lab, strong_labels[strong_labels > 0])


def canny_edges_stack(g: np.ndarray, low: int = 50, high: int = 150) -> np.ndarray:
    """† literal restatement of canny.cpp's single-threaded loop: the map with 0 = may be edge, 1 = not, 2 = edge, the
    prev_flag / upper-neighbour shortcuts of the push, then the stack flood."""
    h, w = g.shape
    dx, dy = sobel(g, replicate=True)
    mag = np.zeros((h + 2, w + 2), np.int64)
    mag[1:-1, 1:-1] = np.abs(dx) + np.abs(dy)
    mp = np.ones((h + 2, w + 2), np.uint8)            # borders: 1 (not edge)
    stack = []
    for i in range(h):
        prev_flag = 0
        for j in range(w):
            m = int(mag[i + 1, j + 1])
            push = False
            if m > low:
                xs, ys = int(dx[i, j]), int(dy[i, j])
                x, y = abs(xs), abs(ys) << 15
                tg22x = x * TG22
                if y < tg22x:
                    push = m > mag[i + 1, j] and m >= mag[i + 1, j + 2]
                else:
                    tg67x = tg22x + (x << 16)
                    if y > tg67x:
                        push = m > mag[i, j + 1] and m >= mag[i + 2, j + 1]
                    else:
                        s = -1 if (xs ^ ys) < 0 else 1
                        push = m > mag[i, j + 1 - s] and m > mag[i + 2, j + 1 + s]
            if push:
                if not prev_flag and m > high and mp[i, j + 1] != 2:
                    mp[i + 1, j + 1] = 2
                    stack.append((i + 1, j + 1))
                    prev_flag = 1
                else:
                    mp[i + 1, j + 1] = 0
                continue
            prev_flag = 0
            mp[i + 1, j + 1] = 1
    while stack:
        y, x = stack.pop()
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                if (oy or ox) and mp[y + oy, x + ox] == 0:
                    mp[y + oy, x + ox] = 2
                    stack.append((y + oy, x + ox))
    return mp[1:-1, 1:-1] == 2


# ---- colour ------------------------------------------------------------------------------------------------------------


def lab_tables_b():
    """† sRGBGammaTab_b[256] (x 255 x 2^3) and LabCbrtTab_b[3072] (x 2^15), fp64, rounded half to even."""
    x = np.arange(256, dtype=np.float64) / 255.0
    gamma = np.rint(255.0 * 8.0 * np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)).astype(np.int64)
    t = np.arange(3072, dtype=np.float64) / (255.0 * 8.0)
    cb = np.rint(32768.0 * np.where(t < 216.0 / 24389.0, t * (841.0 / 108.0) + 16.0 / 116.0, np.cbrt(t))).astype(np.int64)
    return gamma, cb


def lab_coeffs():
    """† round(2^12 sRGB2XYZ_D65[i][j] / D65_white[i]), RGB order."""
    m = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    wp = np.array([0.950456, 1.0, 1.088754])
    return np.rint(4096.0 * m / wp[:, None]).astype(np.int64)


def rgb2lab8(img: np.ndarray) -> np.ndarray:
    gamma, cb = lab_tables_b()
    C = lab_coeffs()
    lin = gamma[img[..., :3].astype(np.int64)]
    f = [cb[(lin @ C[i] + (1 << 11)) >> 12] for i in range(3)]
    L = (296 * f[1] - ((16 * 255 * (1 << 15) + 50) // 100) + (1 << 14)) >> 15
    a = (500 * (f[0] - f[1]) + 128 * (1 << 15) + (1 << 14)) >> 15
    b = (200 * (f[1] - f[2]) + 128 * (1 << 15) + (1 << 14)) >> 15
    return np.clip(np.stack([L, a, b], -1), 0, 255).astype(np.uint8)


def rgb2ycrcb8(img: np.ndarray) -> np.ndarray:
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    Y = (r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14
    Cr = ((r - Y) * 11682 + (128 << 14) + (1 << 13)) >> 14
    Cb = ((b - Y) * 9241 + (128 << 14) + (1 << 13)) >> 14
    return np.clip(np.stack([Y, Cr, Cb], -1), 0, 255).astype(np.uint8)


# ---- the metrics, in the reference's own form ---------------------------------------------------------------------------


def sharpness(g):
    return float(laplacian(g).astype(np.float64).var())


def contrast(g):
    return float(np.std(g.astype(np.float64)))


def hf_ratio(g, fft2=None):
    """fftshift-centred |F| outside radius min(h, w) // 4 over the total (numpy.fft in fp64 unless fft2 is given)."""
    h, w = g.shape
    F = (fft2 or np.fft.fft2)(g.astype(np.float32).astype(np.float64))
    mag = np.abs(np.fft.fftshift(F))
    y, x = np.ogrid[:h, :w]
    mask = (x - w // 2) ** 2 + (y - h // 2) ** 2 > (min(h, w) // 4) ** 2
    return float(mag[mask].sum() / (mag.sum() + 1e-10))


def artifact_score(g):
    h, w = g.shape
    ys, xs = range(0, h - 8, 8), range(0, w - 8, 8)
    v = [np.var(g[y:y + 8, x:x + 8].astype(np.float64)) for y in ys for x in xs] if len(ys) * len(xs) < 200000 else \
        _block_vars_fast(g, len(ys), len(xs))
    if len(v) > 1:
        return float(max(0, 100 - np.var(v) / 100))
    return 100.0


def _block_vars_fast(g, ny, nx):
    b = g[:ny * 8, :nx * 8].astype(np.int64).reshape(ny, 8, nx, 8)
    s, s2 = b.sum((1, 3)), (b * b).sum((1, 3))
    return ((64 * s2 - s * s) / 4096.0).ravel()


def brightness_uniformity(g):
    h, w = g.shape
    rh, rw = h // 4, w // 4
    if rh == 0 or rw == 0:
        return 0.0
    means = [g[i * rh:(i + 1) * rh, j * rw:(j + 1) * rw].astype(np.float64).mean() for i in range(4) for j in range(4)]
    return float(max(0, 100 - np.std(means)))


def noise_level(g):
    n = noise16(g).astype(np.float64) / 16.0
    return float(np.std(n))


def texture(g):
    return float(local_variance5(g).astype(np.float64).mean())


def face_naturalness(img):
    if img.ndim != 3:
        return 50.0
    y = rgb2ycrcb8(img)
    cr, cb = y[..., 1], y[..., 2]
    skin = (cr >= 133) & (cr <= 173) & (cb >= 77) & (cb <= 127)
    return float(np.clip(100 - abs(skin.sum() / skin.size - 0.3) * 100, 0, 100))


def color_variance(img):
    return 0.0 if img.ndim != 3 else float(np.var(rgb2lab8(img)[..., 0].astype(np.float64)))


def colorfulness(img):
    if img.ndim != 3:
        return 0.0
    lab = rgb2lab8(img).astype(np.float64)
    return float(np.sqrt(np.std(lab[..., 1]) ** 2 + np.std(lab[..., 2]) ** 2))


def skin_tone(img):
    if img.ndim != 3:
        return 50.0
    lab = rgb2lab8(img).astype(np.float64)
    d = np.sqrt((lab[..., 0].mean() - 70) ** 2 + (lab[..., 1].mean() - 15) ** 2 + (lab[..., 2].mean() - 20) ** 2)
    return float(max(0, 100 - d))


def delta_e(img, ref):
    if img.ndim != 3:
        return 100.0
    mean_color = img.reshape(-1, img.shape[2]).astype(np.float64).mean(0)
    a = rgb2lab8(np.uint8([[ref]])[..., :3])[0, 0]
    b = rgb2lab8(mean_color.astype(np.uint8)[None, None, :3])[0, 0]
    return float(np.sqrt(np.sum((a.astype(np.float32) - b.astype(np.float32)) ** 2)))


def oversharpen(g):
    e = canny_edges(g)
    return float(max(0, 100 - e.sum() / e.size * 500))


def mscn_stats(g, fp64=True):
    m = mscn(g)
    if fp64:
        d = m.astype(np.float64)
        mean = d.sum() / d.size
        return mean, float(np.sqrt(max((d * d).sum() / d.size - mean * mean, 0.0))), float(np.abs(d).sum() / d.size)
    return float(np.mean(m)), float(np.std(m)), float(np.mean(np.abs(m)))


def niqe(g, fp64=True):
    mean, std, _ = mscn_stats(g, fp64)
    return float(np.clip((std + abs(mean)) * 2.0 + 3.0, 1.0, 15.0))


def brisque(g, fp64=True):
    mean, std, mabs = mscn_stats(g, fp64)
    gx, gy = sobel(g)
    gm = np.sqrt((gx * gx + gy * gy).astype(np.float64))
    return float(np.clip(np.mean([mean, std, mabs, gm.mean(), gm.std()]) * 10 + 20, 0, 100))


def level(v, t):
    ex, gd, fr = t
    return "excellent" if v <= ex else "good" if v <= gd else "fair" if v <= fr else "poor"


def commercial_score(m):
    s = []
    if 'global_sharpness' in m:
        s.append(min(100, m['global_sharpness'] / 10))
    if 'high_frequency_ratio' in m:
        s.append(min(100, m['high_frequency_ratio'] * 500))
    if 'oversharpen_score' in m:
        s.append(m['oversharpen_score'])
    if 'artifact_score' in m:
        s.append(m['artifact_score'])
    return float(np.mean(s)) if s else 50.0


def evaluate_commercial(img, rois=None, gray_shift=15, fft2=None):
    """The reference's evaluate_commercial over the restated rules (key order included)."""
    g = gray_of(img, gray_shift)
    H, W = g.shape
    m = {'global_sharpness': sharpness(g), 'high_frequency_ratio': hf_ratio(g, fft2)}
    boxes = []
    for i, roi in enumerate(rois or []):
        t = roi.get('type', f'roi_{i}')
        x, y, w, h = roi.get('bbox', [0, 0, W, H])
        x, y = max(0, x), max(0, y)
        w, h = min(w, W - x), min(h, H - y)
        boxes.append((i, t, x, y, w, h, roi.get('reference_color')))
    for i, t, x, y, w, h, _ in boxes:
        if w > 0 and h > 0:
            sub, gs = img[y:y + h, x:x + w], g[y:y + h, x:x + w]
            if t == 'text':
                m[f'text_sharpness_{i}'] = sharpness(gs)
                m[f'text_contrast_{i}'] = contrast(gs)
            elif t == 'product':
                m[f'product_texture_{i}'] = texture(gs)
            elif t == 'face':
                m[f'face_naturalness_{i}'] = face_naturalness(sub)
    m['color_variance'] = color_variance(img)
    for i, t, x, y, w, h, ref in boxes:
        if w > 0 and h > 0:
            sub = img[y:y + h, x:x + w]
            if t == 'brand' and ref is not None:
                de = delta_e(sub, ref)
                m[f'brand_color_delta_e_{i}'] = de
                m[f'brand_color_accuracy_{i}'] = level(de, (1.0, 3.0, 5.0))
            elif t == 'face':
                m[f'skin_tone_naturalness_{i}'] = skin_tone(sub)
    m['oversharpen_score'] = oversharpen(g)
    m['artifact_score'] = artifact_score(g)
    m['noise_level'] = noise_level(g)
    m['brightness_uniformity'] = brightness_uniformity(g)
    m['commercial_score'] = commercial_score(m)
    return m


def evaluate_no_reference(img, gray_shift=15, fp64=True):
    g = gray_of(img, gray_shift)
    m = {'niqe': niqe(g, fp64)}
    m['niqe_level'] = level(m['niqe'], (3.0, 5.0, 8.0))
    m['brisque'] = brisque(g, fp64)
    m['brisque_level'] = level(m['brisque'], (20.0, 35.0, 50.0))
    m['sharpness'] = sharpness(g)
    m['contrast'] = contrast(g)
    m['colorfulness'] = colorfulness(img)
    return m


FLOAT_KEYS = ("noise_level", "niqe", "brisque", "product_texture")
HF_KEYS = ("high_frequency_ratio", "commercial_score")


def tolerance(key: str) -> float:
    """Relative bar of one field: 1e-4 for the DFT (and the score that averages it in), 1e-9 for the fp32-map sums,
    1e-12 for everything that comes from exact integer sums."""
    if key.startswith(HF_KEYS):
        return 1e-4
    if key.startswith(FLOAT_KEYS):
        return 1e-9
    return 1e-12
