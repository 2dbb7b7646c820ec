"""NumPy restatement of the reference's ContentAnalyzer (tiling_module.py:261-370 and the per-tile flags of :752-757):
float64 and np.fft in the reference's expression order, every cv2 call pinned to one written-out rule.  Rules marked †
restate OpenCV 4.x from memory (no cv2 on the build machines): they define what the HIP kernels compute and cannot be
checked against OpenCV itself here.

  gray †          cv2.COLOR_BGR2GRAY applied to the RGB data the pipeline carries: descale(B' 3735 + G 19235 + R' 9798, 15)
                  with B' = channel 0, R' = channel 2 (the swapped-weight rule split_array's complexity_score uses)
  filter2D †      default border BORDER_REFLECT_101 and centred anchor; the 5x5 kernel of 1/25 is a correlation whose
                  float64 terms k * v are added one after the other
  GaussianBlur †  ksize 5, sigma 0: OpenCV's small fixed table [1 4 6 4 1] / 16, separable (rows, then columns),
                  BORDER_REFLECT_101
  calcHist †      256 bins of [0, 256) with float32 counts, so hist / hist.sum() and the entropy sum are float32
  reflect-101     np.pad(mode="reflect"); a length-1 axis repeats its value (borderInterpolate's answer); widths above
                  n - 1 reflect repeatedly
`dtype` switches the real / complex type the saliency is evaluated in (float64: the reference; float32: the same
expressions in complex64, the yardstick for what single precision costs).
"""
from __future__ import annotations

import numpy as np


def gray_bgr_rule(img: np.ndarray) -> np.ndarray:
    """† COLOR_BGR2GRAY on RGB data; 2-D (or one-channel) input is its own gray plane."""
    if img.ndim == 2:
        return img.copy()
    if img.shape[2] == 1:
        return img[..., 0].copy()
    t = img.astype(np.int64)
    return ((t[..., 0] * 3735 + t[..., 1] * 19235 + t[..., 2] * 9798 + (1 << 14)) >> 15).astype(np.uint8)


def pad101(a: np.ndarray, p: int) -> np.ndarray:
    for ax in range(a.ndim):
        n = a.shape[ax]
        left = p
        while left > 0:                      # np.pad reflects at most n - 1 at a time
            step = left if n == 1 else min(left, n - 1)
            width = [(0, 0)] * a.ndim
            width[ax] = (step, step)
            a = np.pad(a, width, mode="reflect" if n > 1 else "edge")
            left -= step
            n = a.shape[ax]
    return a


def box5_mean(L: np.ndarray) -> np.ndarray:
    """† cv2.filter2D(L, -1, ones((5, 5)) / 25)."""
    h, w = L.shape
    P = pad101(L, 2)
    k = L.dtype.type(1.0) / L.dtype.type(25.0)
    acc = np.zeros_like(L)
    for i in range(5):
        for j in range(5):
            acc = acc + k * P[i:i + h, j:j + w]
    return acc


def gauss5(S: np.ndarray) -> np.ndarray:
    """† cv2.GaussianBlur(S, (5, 5), 0)."""
    h, w = S.shape
    k = (np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0).astype(S.dtype)
    P = pad101(S, 2)
    rows = sum(k[j] * P[:, j:j + w] for j in range(5))
    return sum(k[i] * rows[i:i + h, :] for i in range(5))


def saliency_float(image: np.ndarray, dtype=np.float64) -> np.ndarray:
    """The blurred saliency before normalisation (tiling_module.py:261-285)."""
    real = np.dtype(dtype)
    cplx = np.complex128 if real == np.float64 else np.complex64
    gray = gray_bgr_rule(image)
    f = np.fft.fft2(gray.astype(cplx))
    fshift = np.fft.fftshift(f)
    magnitude = np.abs(fshift)
    log_magnitude = np.log(magnitude + real.type(1e-8))
    avg = box5_mean(log_magnitude)
    spectral_residual = log_magnitude - avg
    phase = np.angle(fshift)
    saliency_complex = np.exp(spectral_residual + 1j * phase).astype(cplx)
    sal = np.abs(np.fft.ifft2(np.fft.ifftshift(saliency_complex)))
    assert sal.dtype == real, sal.dtype
    return gauss5(sal)


def normalise_u8(s: np.ndarray) -> np.ndarray:
    """tiling_module.py:286-287."""
    return ((s - s.min()) / (s.max() - s.min() + s.dtype.type(1e-8)) * 255).astype(np.uint8)


def saliency(image: np.ndarray, dtype=np.float64) -> np.ndarray:
    return normalise_u8(saliency_float(image, dtype))


def min_spectrum_magnitude(image: np.ndarray) -> float:
    return float(np.abs(np.fft.fft2(gray_bgr_rule(image).astype(np.float64))).min())


def local_entropy(image: np.ndarray, window_size: int = 64) -> np.ndarray:
    """tiling_module.py:291-321 († calcHist: float32 counts)."""
    gray = gray_bgr_rule(image)
    out = np.zeros(gray.shape, dtype=np.float32)
    for y in range(0, gray.shape[0], window_size):
        for x in range(0, gray.shape[1], window_size):
            win = gray[y:min(y + window_size, gray.shape[0]), x:min(x + window_size, gray.shape[1])]
            hist = np.bincount(win.ravel(), minlength=256).astype(np.float32)
            hist = hist / hist.sum()
            ent = -np.sum(hist * np.log2(hist + np.float32(1e-10)))
            assert ent.dtype == np.float32
            out[y:min(y + window_size, gray.shape[0]), x:min(x + window_size, gray.shape[1])] = ent
    return out


def forbidden_map(image: np.ndarray, faces=(), texts=None, protect_salient: bool = True, saliency_threshold: float = 0.7,
                  saliency_map: np.ndarray = None) -> np.ndarray:
    """tiling_module.py:344-370 with the detectors' boxes given (texts None: protect_text off)."""
    h, w = image.shape[:2]
    fm = np.zeros((h, w), dtype=bool)
    for x, y, bw, bh in faces:
        margin = int(max(bw, bh) * 0.2)
        x1, y1 = max(0, x - margin), max(0, y - margin)
        x2, y2 = min(w, x + bw + margin), min(h, y + bh + margin)
        fm[y1:y2, x1:x2] = True
    for x, y, bw, bh in (texts or ()):
        fm[y:y + bh, x:x + bw] = True
    if protect_salient:
        sal = saliency(image) if saliency_map is None else saliency_map
        fm |= sal > int(255 * saliency_threshold)
    return fm


def tile_flags(fm: np.ndarray, positions) -> list:
    """tiling_module.py:752-757."""
    out = []
    for x, y, w, h in positions:
        t = fm[y:y + h, x:x + w]
        out.append({'has_forbidden_zone': bool(np.any(t)), 'forbidden_ratio': float(np.sum(t) / t.size)})
    return out


# (h, w, cn) of the GPU saliency tests: powers of two, odd sides, prime sides (257, 193, 769, 1021 are single direct-DFT
# passes; 1031 > 1024 takes the Bluestein path), one-pixel-wide / -tall images, every channel count
SALIENCY_CASES = [(64, 64, 3), (256, 128, 3), (257, 384, 3), (255, 301, 3), (257, 193, 3), (1021, 769, 3), (1031, 520, 3),
                  (1, 300, 3), (300, 1, 3), (120, 200, 1), (120, 200, 4), (512, 768, 3), (1000, 1500, 3)]


def synthetic(h: int, w: int, cn: int = 3, seed: int = 10) -> np.ndarray:
    """Smooth structure + a compact bright object + noise: a non-degenerate spectrum and a salient spot."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 96 + 40 * np.sin(xx / 37.0 + 0.3) + 30 * np.cos(yy / 23.0) + 10 * np.sin((xx + 2 * yy) / 61.0)
    cy, cx = 0.37 * (h - 1), 0.61 * (w - 1)
    ry, rx = max(1.0, 0.04 * h), max(1.0, 0.04 * w)
    blob = 110 * np.exp(-(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2))
    planes = []
    for c in range(3 if cn >= 3 else 1):
        planes.append(base * (1.0 - 0.08 * c) + blob * (1.0 + 0.1 * c) + rng.integers(-12, 13, (h, w)))
    img = np.clip(np.stack(planes, axis=-1), 0, 255).astype(np.uint8)
    if cn == 4:
        img = np.concatenate([img, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=-1)
    if cn == 1:
        return img[..., 0]
    return img
