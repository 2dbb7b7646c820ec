"""Plain-NumPy restatement of BlendingModule.gradient_domain_fusion (reference blending_module.py:1377-1523) and of the
module-level compute_blend_quality (:1563-1608), for the tests.  cv2 is not installed: cv2.Sobel(ksize=3, BORDER_DEFAULT)
is restated in OpenCV's separable order -- the row kernel first, then the column kernel, derivative [-1, 0, 1] = b - a,
smoothing [1, 2, 1] = (a + c) + 2 b -- in float32 on reflect-101 padding.  Exact for integer-valued data; for other float
data this order is the one the HIP kernels follow (parity with OpenCV unpinned)."""
from __future__ import annotations

import numpy as np

from oracle import oracle_np as onp


def sobel_f32(img: np.ndarray):
    """cv2.Sobel(img, CV_32F, 1, 0, ksize=3) and (0, 1) of one 2-D channel -> (gx, gy) float32."""
    a = np.asarray(img, dtype=np.float32)
    p = np.pad(a, 1, mode="reflect")                # NumPy's 'reflect' is reflect-101 (the edge is not repeated)
    d = p[:, 2:] - p[:, :-2]                        # row pass of gx: [-1, 0, 1]
    gx = (d[:-2] + d[2:]) + np.float32(2) * d[1:-1]
    s = (p[:, :-2] + p[:, 2:]) + np.float32(2) * p[:, 1:-1]   # row pass of gy: [1, 2, 1]
    gy = s[2:] - s[:-2]
    return gx, gy


def weight_map(h: int, w: int) -> np.ndarray:
    """_create_distance_weight_map(h, w, COSINE) (:508-561), float32."""
    fw = min(h, w) // 8
    y = np.arange(h).reshape(-1, 1)
    x = np.arange(w).reshape(1, -1)
    d = np.minimum(np.minimum(y, h - 1 - y), np.minimum(x, w - 1 - x))
    nd = np.clip(d / fw, 0, 1)
    return (0.5 * (1 - np.cos(np.pi * nd))).astype(np.float32)


def _tile_gradients(tile: np.ndarray):
    t = tile if tile.dtype == np.float32 else tile.astype(np.float32)
    if t.ndim == 2:
        return sobel_f32(t)
    gx, gy = np.zeros_like(t), np.zeros_like(t)
    for c in range(t.shape[2]):
        gx[:, :, c], gy[:, :, c] = sobel_f32(t[:, :, c])
    return gx, gy


def _normalised_gradients(tiles, positions, output_shape):
    """The weighted, list-ordered float32 accumulation of gradient_domain_fusion -> (grad_x / W, grad_y / W)."""
    H, W = output_shape
    cn = tiles[0].shape[2] if tiles[0].ndim == 3 else 1
    shape = (H, W) if cn == 1 else (H, W, cn)
    grad_x = np.zeros(shape, np.float32)
    grad_y = np.zeros(shape, np.float32)
    wacc = np.zeros((H, W), np.float32)
    for tile, (y, x) in zip(tiles, positions):
        h, w = tile.shape[:2]
        gx, gy = _tile_gradients(tile)
        wt = weight_map(h, w)
        ye, xe = min(y + h, H), min(x + w, W)
        wc = wt[:ye - y, :xe - x]
        wb = wc[..., None] if cn > 1 else wc
        grad_x[y:ye, x:xe] += gx[:ye - y, :xe - x] * wb
        grad_y[y:ye, x:xe] += gy[:ye - y, :xe - x] * wb
        wacc[y:ye, x:xe] += wc
    wacc = np.maximum(wacc, 1e-6)
    wb = wacc[..., None] if cn > 1 else wacc
    grad_x /= wb
    grad_y /= wb
    return grad_x, grad_y


def gradient_domain_fusion(tiles, positions, output_shape) -> np.ndarray:
    """The reference's sequence of float32 array operations, vectorised as it is there."""
    grad_x, grad_y = _normalised_gradients(tiles, positions, output_shape)
    r = np.cumsum(grad_x, axis=1)
    r += np.cumsum(grad_y, axis=0)
    r /= 2
    return np.clip(r, 0, 255).astype(np.uint8)


def row_prefix_plane(tiles, positions, output_shape) -> np.ndarray:
    """np.cumsum(grad_x / max(wacc, 1e-6), axis=1) in float32: the first half of gradient_domain_fusion, the plane
    sr_gradient_fusion leaves in its workspace.  The u8 canvas hides most fp32 differences; this plane does not."""
    grad_x, _ = _normalised_gradients(tiles, positions, output_shape)
    return np.cumsum(grad_x, axis=1)


def gradient_domain_fusion_loops(tiles, positions, output_shape) -> np.ndarray:
    """The same contract written as explicit float32 scalar loops (small grids only): pins that the vectorised form above
    is the sequential, list-ordered fp32 evaluation the kernels implement."""
    H, W = output_shape
    cn = tiles[0].shape[2] if tiles[0].ndim == 3 else 1
    f = np.float32
    gx_acc = np.zeros((H, W, cn), np.float32)
    gy_acc = np.zeros((H, W, cn), np.float32)
    wacc = np.zeros((H, W), np.float32)
    for tile, (y, x) in zip(tiles, positions):
        t = tile.astype(np.float32).reshape(tile.shape[0], tile.shape[1], cn)
        h, w = t.shape[:2]
        wt = weight_map(h, w)

        def ref(p, n):
            return -p if p < 0 else (2 * n - 2 - p if p >= n else p)
        for ly in range(min(h, H - y)):
            for lx in range(min(w, W - x)):
                ym, yp, xm, xp = ref(ly - 1, h), ref(ly + 1, h), ref(lx - 1, w), ref(lx + 1, w)
                for c in range(cn):
                    d = [f(t[r, xp, c] - t[r, xm, c]) for r in (ym, ly, yp)]
                    gx = f(f(d[0] + d[2]) + f(f(2) * d[1]))
                    s = [f(f(t[r, xm, c] + t[r, xp, c]) + f(f(2) * t[r, lx, c])) for r in (ym, yp)]
                    gy = f(s[1] - s[0])
                    gx_acc[y + ly, x + lx, c] = f(gx_acc[y + ly, x + lx, c] + f(gx * wt[ly, lx]))
                    gy_acc[y + ly, x + lx, c] = f(gy_acc[y + ly, x + lx, c] + f(gy * wt[ly, lx]))
                wacc[y + ly, x + lx] = f(wacc[y + ly, x + lx] + wt[ly, lx])
    out = np.zeros((H, W, cn), np.uint8)
    for c in range(cn):
        cx = np.zeros((H, W), np.float32)
        for i in range(H):
            run = f(0)
            for j in range(W):
                run = f(run + f(gx_acc[i, j, c] / max(wacc[i, j], f(1e-6))))
                cx[i, j] = run
        for j in range(W):
            run = f(0)
            for i in range(H):
                run = f(run + f(gy_acc[i, j, c] / max(wacc[i, j], f(1e-6))))
                v = f(f(cx[i, j] + run) / f(2))
                out[i, j, c] = int(min(max(v, f(0)), f(255)))
    return out[:, :, 0] if tiles[0].ndim == 2 else out


def _ssim_gray(a: np.ndarray, b: np.ndarray) -> float:
    """_compute_ssim (:855-903): BGR2GRAY of 3-D data, float64 global statistics."""
    g1 = onp.bgr2gray_on_rgb_u8(a[..., :3] if a.ndim == 3 else a).astype(np.float64)
    g2 = onp.bgr2gray_on_rgb_u8(b[..., :3] if b.ndim == 3 else b).astype(np.float64)
    mu1, mu2 = np.mean(g1), np.mean(g2)
    s1, s2 = np.var(g1), np.var(g2)
    s12 = np.mean((g1 - mu1) * (g2 - mu2))
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    return float(((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 ** 2 + mu2 ** 2 + c1) * (s1 + s2 + c2)))


def _resize_u8(tile: np.ndarray, w: int, h: int) -> np.ndarray:
    if tile.ndim == 2:
        return onp.resize_linear_u8(tile[..., None], w, h)[..., 0]
    return onp.resize_linear_u8(tile, w, h)


def _magnitude(result: np.ndarray, dtype):
    r = result if result.ndim == 3 else result[..., None]
    mags = []
    for c in range(r.shape[2]):
        gx, gy = sobel_f32(r[:, :, c])
        gx, gy = gx.astype(dtype), gy.astype(dtype)
        mags.append(np.sqrt(gx ** 2 + gy ** 2))
    return np.stack(mags, axis=-1)


def compute_blend_quality(result, tiles, positions, literal: bool = False) -> dict:
    """float64 restatement (literal=True: the gradient fields as the reference's float32 expressions)."""
    scores = []
    for tile, (y, x) in zip(tiles, positions):
        h, w = tile.shape[:2]
        roi = result[y:y + h, x:x + w]
        if roi.shape != tile.shape:
            tile = _resize_u8(tile, roi.shape[1], roi.shape[0])
        scores.append(_ssim_gray(roi, tile))
    m = _magnitude(result, np.float32 if literal else np.float64)
    return {"mean_ssim": np.mean(scores), "min_ssim": np.min(scores), "std_ssim": np.std(scores),
            "mean_gradient": np.mean(m), "gradient_discontinuity": np.std(m)}
