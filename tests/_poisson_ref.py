"""NumPy / SciPy restatement of BlendingModule.poisson_fusion and repair_seams (reference blending_module.py:563-659,
1148-1240): what the HIP kernels of csrc/sr_poisson.hip compute, written out from the rules below.  Rules marked † restate
OpenCV 4.x from memory (no cv2 on the build machines): they define the behaviour and cannot be checked against OpenCV here.

  seamlessClone †  the mask's outer 1-pixel frame is zeroed, roi_s = bounding rectangle of what is left, roi_d the rectangle
                   of the same size at (cx - roi_s.w // 2, cy - roi_s.h // 2) in the destination; the patch is src[roi_s] with
                   the pixels outside the mask zeroed; Cloning::normalClone runs on that one rectangle
  normalClone †    mask = (mask != 0) eroded three times by a 3 x 3 element, the outside not eroding; forward differences of
                   destination and patch; patch pair under the mask (MIXED: per pixel and channel the pair with the larger
                   |gx - gy|; MONOCHROME: the patch is its 8-bit RGB2GRAY value in all channels), destination pair elsewhere;
                   backward differences give the Laplacian; the 4-neighbour Laplacian of the destination with its interior
                   zeroed is subtracted; DST-I, division by (2 cos(pi (x + 1) / (w - 1)) - 2) + (2 cos(pi (y + 1) / (h - 1)) - 2),
                   inverse DST-I; saturate(round-half-even) into the interior, the frame is the destination's
  GaussianBlur †   (15, 15), sigma 0 -> 2.6; 8.8 fixed-point taps (side taps rounded, the centre takes what is left of 256:
                   BLUR15_TAPS), the row pass exact, the column pass rounded once ((s + 2^15) >> 16), BORDER_REFLECT_101
  RGB2GRAY †       (R 9798 + G 19235 + B 3735 + 2^14) >> 15
`dtype` is the type the solve runs in: float64 is the reference value, float32 the yardstick for what single precision costs.
"""
from __future__ import annotations

import numpy as np
from scipy import fft as sfft
from scipy import ndimage as ndi

from oracle import oracle_np as onp

NORMAL, MIXED, MONOCHROME = 1, 2, 3
# † getGaussianKernel(15, 2.6) * 256: 1.051 2.750 6.205 12.073 20.262 29.329 36.616 39.426 ...
BLUR15_TAPS = np.array([1, 3, 6, 12, 20, 29, 37, 40, 37, 29, 20, 12, 6, 3, 1], dtype=np.int64)

SOLVER_CASES = [(64, 96), (301, 407), (1032, 517), (1024, 1536)]


def synth(h: int, w: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((h, w, 3), np.float64)
    for c in range(3):
        out[..., c] = 128 + 64 * np.sin(x / 37 + c + seed) + 48 * np.cos(y / 23 + 2 * c) + rng.integers(-12, 13, (h, w))
    return np.clip(out, 0, 255).astype(np.uint8)


def solver_inputs(h: int, w: int):
    """Destination, a brighter unrelated patch and a centred box mask (the inputs of the CPU precision probe)."""
    dest = synth(h, w, 1)
    patch = np.clip(synth(h, w, 2).astype(int) + 25, 0, 255).astype(np.uint8)
    mask = np.zeros((h, w), np.uint8)
    mask[h // 6:h - h // 6, w // 6:w - w // 6] = 255
    return dest, patch, mask


def rgb2gray(img: np.ndarray) -> np.ndarray:
    t = img.astype(np.int64)
    return ((t[..., 0] * 9798 + t[..., 1] * 19235 + t[..., 2] * 3735 + (1 << 14)) >> 15).astype(np.uint8)


def eroded_mask(mask: np.ndarray) -> np.ndarray:
    return ndi.binary_erosion(mask != 0, np.ones((3, 3), bool), iterations=3, border_value=1)


def guidance(dest: np.ndarray, patch: np.ndarray, mask: np.ndarray, mode: int, dtype=np.float64):
    """-> (right-hand side of the interior problem, (h - 2, w - 2, 3); Laplacian of the guidance field alone)."""
    m = eroded_mask(mask).astype(dtype)[..., None]
    d = dest.astype(dtype)
    s = patch
    if mode == MONOCHROME:
        s = np.repeat(rgb2gray(patch)[..., None], 3, axis=2)
    s = s.astype(dtype)

    def fwd(a, ax):                                        # I[i + 1] - I[i]; the last one is never read
        out = np.zeros_like(a)
        sl = [slice(None)] * 3
        sl[ax] = slice(0, -1)
        out[tuple(sl)] = np.diff(a, axis=ax)
        return out

    dgx, dgy, pgx, pgy = fwd(d, 1), fwd(d, 0), fwd(s, 1), fwd(s, 0)
    if mode == MIXED:
        pick = np.abs(pgx - pgy) > np.abs(dgx - dgy)
        pgx, pgy = np.where(pick, pgx, dgx), np.where(pick, pgy, dgy)
    fx = dgx * (1 - m) + pgx * m
    fy = dgy * (1 - m) + pgy * m
    lap = np.zeros_like(fx)
    lap[:, 1:] += fx[:, 1:] - fx[:, :-1]                   # g[i] - g[i - 1]
    lap[1:, :] += fy[1:, :] - fy[:-1, :]
    b = d.copy()
    b[1:-1, 1:-1] = 0
    bl = b[1:-1, :-2] + b[1:-1, 2:] + b[:-2, 1:-1] + b[2:, 1:-1]          # the centre is interior: zero
    return (lap[1:-1, 1:-1] - bl).astype(dtype), lap[1:-1, 1:-1]


def solve(rhs: np.ndarray, dtype=np.float64) -> np.ndarray:
    hi, wi = rhs.shape[:2]
    ky = (2 * np.cos(np.pi * (np.arange(hi) + 1) / (hi + 1)) - 2).astype(dtype)[:, None, None]
    kx = (2 * np.cos(np.pi * (np.arange(wi) + 1) / (wi + 1)) - 2).astype(dtype)[None, :, None]
    t = sfft.dstn(rhs.astype(dtype), type=1, axes=(0, 1))
    t = (t / (ky + kx)).astype(dtype)
    return sfft.idstn(t, type=1, axes=(0, 1)).astype(dtype)


def clone(dest: np.ndarray, patch: np.ndarray, mask: np.ndarray, mode: int = NORMAL, dtype=np.float64, raw: bool = False):
    """† Cloning::normalClone on one rectangle.  raw: also the solution before rounding."""
    h, w = mask.shape
    out = dest.copy()
    if h < 3 or w < 3:
        return (out, None) if raw else out
    rhs, _ = guidance(dest, patch, mask, mode, dtype)
    r = solve(rhs, dtype)
    out[1:-1, 1:-1] = np.clip(np.rint(r), 0, 255).astype(np.uint8)
    return (out, r) if raw else out


def dst1_by_fft(x: np.ndarray) -> np.ndarray:
    """DST-I (SciPy's scale: 2 sum x sin) from the DFT of the odd extension to 2 (n + 1): -Im F[1..n]."""
    n = x.shape[-1]
    ext = np.zeros(x.shape[:-1] + (2 * (n + 1),), x.dtype)
    ext[..., 1:n + 1] = x
    ext[..., n + 2:] = -x[..., ::-1]
    return -np.fft.fft(ext, axis=-1).imag[..., 1:n + 1]


def clone_rects(mask: np.ndarray, dst_shape, center):
    """† seamlessClone's rectangles -> ((x, y, w, h) roi_s, (x, y, w, h) roi_d), or None when the mask is empty after its
    frame is zeroed or roi_d leaves the destination."""
    m = mask != 0
    m[0, :] = m[-1, :] = False
    m[:, 0] = m[:, -1] = False
    ys, xs = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
    if ys.size == 0:
        return None
    x0, y0, rw, rh = int(xs[0]), int(ys[0]), int(xs[-1] - xs[0] + 1), int(ys[-1] - ys[0] + 1)
    dx, dy = int(center[0]) - rw // 2, int(center[1]) - rh // 2
    if dx < 0 or dy < 0 or dx + rw > dst_shape[1] or dy + rh > dst_shape[0]:
        return None
    return (x0, y0, rw, rh), (dx, dy, rw, rh)


def fallback_blend(src, dst, mask, center):
    """blending_module.py:627-659: float32 roi (1 - m) + src m, truncated to uint8."""
    h, w = src.shape[:2]
    cx, cy = center
    x1, y1 = max(0, cx - w // 2), max(0, cy - h // 2)
    x2, y2 = min(dst.shape[1], x1 + w), min(dst.shape[0], y1 + h)
    s = src[:y2 - y1, :x2 - x1]
    m = mask[:y2 - y1, :x2 - x1].astype(np.float32) / 255.0
    if s.ndim == 3:
        m = m[..., None]
    out = dst.copy()
    out[y1:y2, x1:x2] = (out[y1:y2, x1:x2] * (1 - m) + s * m).astype(np.uint8)
    return out


def poisson_fusion(src, dst, mask=None, center=None, mode: int = NORMAL, dtype=np.float64):
    """blending_module.py:563-625 with cv2.seamlessClone restated; what OpenCV would reject takes fallback_blend."""
    if src.dtype != np.uint8:
        src = np.clip(src, 0, 255).astype(np.uint8)
    if dst.dtype != np.uint8:
        dst = np.clip(dst, 0, 255).astype(np.uint8)
    if mask is None:
        mask = np.ones(src.shape[:2], np.uint8) * 255
    elif mask.dtype != np.uint8:
        mask = (mask > 0).astype(np.uint8) * 255
    if center is None:
        center = (dst.shape[1] // 2, dst.shape[0] // 2)
    ok = src.ndim == 3 and dst.ndim == 3 and src.shape[2] == 3 and dst.shape[2] == 3 and mask.shape == src.shape[:2]
    rects = clone_rects(mask.copy(), dst.shape, center) if ok else None
    if rects is None:
        if ok and not mask.any():
            return dst.copy()
        return fallback_blend(src, dst, mask, center)
    (sx, sy, rw, rh), (dx, dy, _, _) = rects
    mroi = mask[sy:sy + rh, sx:sx + rw]
    patch = src[sy:sy + rh, sx:sx + rw] * (mroi != 0)[..., None].astype(np.uint8)
    out = dst.copy()
    out[dy:dy + rh, dx:dx + rw] = clone(dst[dy:dy + rh, dx:dx + rw], patch, mroi, mode, dtype)
    return out


def _reflect101(idx: np.ndarray, n: int) -> np.ndarray:
    if n == 1:
        return np.zeros_like(idx)
    idx = idx.copy()
    while True:
        bad = (idx < 0) | (idx >= n)
        if not bad.any():
            return idx
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= n, 2 * n - 2 - idx, idx)


def gaussian_blur15(img: np.ndarray) -> np.ndarray:
    """† cv2.GaussianBlur(img, (15, 15), 0) on uint8."""
    a = img.astype(np.int64)
    h, w = a.shape[:2]
    rows = sum(int(BLUR15_TAPS[t]) * a[:, _reflect101(np.arange(w) + t - 7, w)] for t in range(15))
    cols = sum(int(BLUR15_TAPS[t]) * rows[_reflect101(np.arange(h) + t - 7, h)] for t in range(15))
    return ((cols + (1 << 15)) >> 16).astype(np.uint8)


def region_ssim(a: np.ndarray, b: np.ndarray) -> float:
    """_compute_ssim (blending_module.py:855-903) in float64; gray is BGR2GRAY applied to the RGB data."""
    g1 = onp.bgr2gray_on_rgb_u8(a).astype(np.float64)
    g2 = onp.bgr2gray_on_rgb_u8(b).astype(np.float64)
    mu1, mu2 = np.mean(g1), np.mean(g2)
    s12 = np.mean((g1 - mu1) * (g2 - mu2))
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    return float(((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 ** 2 + mu2 ** 2 + c1) * (np.var(g1) + np.var(g2) + c2)))


def best_tile(region: np.ndarray, tiles) -> np.ndarray:
    """_find_best_matching_tile (:1218-1240): the first tile of the largest score, resized to the region."""
    h, w = region.shape[:2]
    best, best_score = tiles[0], -1
    for t in tiles:
        score = region_ssim(region, onp.resize_linear_u8(t, w, h))
        if score > best_score:
            best, best_score = t, score
    return onp.resize_linear_u8(best, w, h)


def padded_box(seam, shape):
    x1, y1 = seam.x, seam.y
    x2, y2 = x1 + seam.width, y1 + seam.height
    pad = max(seam.width, seam.height)
    return max(0, x1 - pad), max(0, y1 - pad), min(shape[1], x2 + pad), min(shape[0], y2 + pad)


def repair_seams(image, seams, tiles, repair_method: str = "auto", dtype=np.float64):
    """blending_module.py:1148-1216, seams in list order on one working copy."""
    out = image.copy()
    for s in seams:
        method = s.suggested_fix if repair_method == "auto" else repair_method
        if method == "none":
            continue
        xa, ya, xb, yb = padded_box(s, image.shape)
        roi = out[ya:yb, xa:xb].copy()
        if method == "increase_blend_width":
            roi = gaussian_blur15(roi)
        elif method == "poisson_refinement":
            mask = np.zeros((yb - ya, xb - xa), np.uint8)
            mask[s.y - ya:s.y + s.height - ya, s.x - xa:s.x + s.width - xa] = 255
            best = best_tile(roi, tiles)
            roi = poisson_fusion(best[:yb - ya, :xb - xa], roi, mask, ((xb - xa) // 2, (yb - ya) // 2), MIXED, dtype)
        out[ya:yb, xa:xb] = roi
    return out
