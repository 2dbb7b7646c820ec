"""NumPy restatement of MATLAB's bicubic imresize as include/sr_hip.h defines it (the form BasicSR's matlab_functions.imresize
restates): float64 throughout, taps added in ascending order, no intermediate rounding.  Written from the header's text, not
from the library's code; the tests hold the library against it."""
import math

import numpy as np

SCALES = (1 / 2, 1 / 3, 1 / 4, 1 / 8, 1 / 16, 3 / 4, 1, 1.5, 2, 3, 4)


def cubic(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    near = 1.5 * (x * x * x) - 2.5 * (x * x) + 1.0
    far = -0.5 * (x * x * x) + 2.5 * (x * x) - 4.0 * x + 2.0
    return np.where(x <= 1.0, near, np.where(x <= 2.0, far, 0.0))


def out_size(n: int, scale: float) -> int:
    return int(math.ceil(n * scale))


def geometry(h: int, w: int, scale=None, output_shape=None):
    """-> (scale_y, scale_x, dh, dw) of the two forms of the size argument."""
    if scale is not None:
        return float(scale), float(scale), out_size(h, scale), out_size(w, scale)
    dh, dw = output_shape
    return dh / h, dw / w, int(dh), int(dw)


def reflect(idx1, n: int):
    """1-based unreflected indices -> 0-based indices under MATLAB's symmetric padding, any distance."""
    j = np.mod(np.asarray(idx1, dtype=np.int64) - 1, 2 * n)
    return np.where(j >= n, 2 * n - 1 - j, j)


def weights(n_in: int, n_out: int, scale: float, antialias: bool = True):
    """(w[n_out, taps] float64, idx[n_out, taps] int64): the normalised weights and reflected 0-based indices; leading and
    trailing taps that are zero for every output are dropped."""
    shrink = antialias and scale < 1
    kw = 4.0 / scale if shrink else 4.0
    P = int(math.ceil(kw)) + 2
    w = np.zeros((n_out, P), dtype=np.float64)
    idx = np.zeros((n_out, P), dtype=np.int64)
    for i in range(n_out):
        u = (i + 1) / scale + 0.5 * (1.0 - 1.0 / scale)
        left = math.floor(u - kw / 2.0)
        total = 0.0
        for k in range(P):
            d = u - left - k
            w[i, k] = scale * float(cubic(scale * d)) if shrink else float(cubic(d))
            total += w[i, k]
            idx[i, k] = left + k
        w[i] /= total
    keep = np.flatnonzero(np.any(w != 0.0, axis=0))
    c0, c1 = int(keep[0]), int(keep[-1])
    return w[:, c0:c1 + 1].copy(), reflect(idx[:, c0:c1 + 1], n_in)


def _pass(a: np.ndarray, w: np.ndarray, idx: np.ndarray, axis: int) -> np.ndarray:
    out = None
    for k in range(w.shape[1]):
        shape = [1] * a.ndim
        shape[axis] = -1
        term = w[:, k].reshape(shape) * np.take(a, idx[:, k], axis=axis)
        out = 0.0 + term if out is None else out + term
    return out


def imresize_f64(image: np.ndarray, scale=None, output_shape=None, antialias: bool = True) -> np.ndarray:
    """The unclamped float64 result in gray levels of a u8 image H x W or H x W x C."""
    a = np.asarray(image).astype(np.float64)
    h, w = a.shape[:2]
    sy, sx, dh, dw = geometry(h, w, scale, output_shape)
    wy, iy = weights(h, dh, sy, antialias)
    wx, ix = weights(w, dw, sx, antialias)
    if sy <= sx:                                        # the smaller scale first; a tie: the vertical pass
        return _pass(_pass(a, wy, iy, 0), wx, ix, 1)
    return _pass(_pass(a, wx, ix, 1), wy, iy, 0)


def to_u8(v: np.ndarray) -> np.ndarray:
    return np.minimum(255.0, np.maximum(0.0, np.floor(v + 0.5))).astype(np.uint8)


def half_distance(v: np.ndarray) -> np.ndarray:
    """|v - (the nearest k + 1/2)|: how far each value is from a rounding tie."""
    return np.abs(v - np.floor(v) - 0.5)
