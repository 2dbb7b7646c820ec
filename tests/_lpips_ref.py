"""LPIPS with spatial output, in float64 and float32 -- TEST INFRASTRUCTURE ONLY.

oracle/lpips_oracle.py returns five spatial means in float32; the small-shape GPU tests (test_gpu_lpips_small.py) need the five
per-pixel ``lin`` maps, in float64 as the reference and in float32 to measure what float32 arithmetic in another summation
order costs.  This file restates the same published forward (ARCH, synthetic_weights and to_lpips_tensor are the oracle's) with
the dtype as an argument and no spatial reduction, and restates -- independently of csrc/sr_vgg_ranges.h -- which cell of a
tap's map a tile of the input owns."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from oracle import lpips_oracle as lo

ARCH = lo.ARCH
synthetic_weights = lo.synthetic_weights
to_lpips_tensor = lo.to_lpips_tensor


def pair(rng, h: int, w: int, cn: int = 3, sigma: float = 9.0):
    """Seeded u8 image pair (cn 0: gray HW): waves of about 7 px (x) and 5 px (y) period so that a 16 x 16 image is not flat,
    +-20 of noise, and b = a + N(0, sigma)."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 64 * np.sin(xx * (2 * np.pi / 7.0)) + 48 * np.cos(yy * (2 * np.pi / 5.0))
    shape = (h, w) if cn == 0 else (h, w, cn)
    base = base if cn == 0 else base[..., None]
    a = np.clip(base + rng.integers(-20, 21, shape), 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.float32) + rng.normal(0, sigma, shape), 0, 255).astype(np.uint8)
    return a, b


def _input(image: np.ndarray, dtype):
    """The network input before the ScalingLayer.  float32: the oracle's to_lpips_tensor as it is.  float64: the same rule (gray
    repeated, alpha dropped, / 255, x 2 - 1) on float64 values."""
    import torch
    if dtype == torch.float32:
        return to_lpips_tensor(image)
    img = image.astype(np.float64) / 255.0
    if img.ndim == 2:
        img = np.stack([img, img, img], axis=-1)
    elif img.shape[2] == 1:
        img = np.repeat(img, 3, axis=-1)
    elif img.shape[2] == 4:
        img = img[:, :, :3]
    return torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).unsqueeze(0) * 2.0 - 1.0


def lin_maps(img1: np.ndarray, img2: np.ndarray, net: str, weights: Dict[str, np.ndarray], dtype: str = "float64") -> List[np.ndarray]:
    """The five per-pixel lin maps, each (H_k, W_k) float64 (float32 arithmetic when dtype is "float32", widened at the end):
    m.sum() is what sr_lpips_u8 returns for the tap, m.mean() the oracle's per-tap value.  The constants (shift, scale, weights)
    are the float32 values the GPU is given, widened exactly."""
    import torch
    import torch.nn.functional as F
    dt = {"float64": torch.float64, "float32": torch.float32}[dtype]
    shift = torch.tensor(lo.SHIFT, dtype=torch.float32).view(1, 3, 1, 1).to(dt)
    scale = torch.tensor(lo.SCALE, dtype=torch.float32).view(1, 3, 1, 1).to(dt)
    maps = []
    with torch.no_grad():
        xs = [(_input(im, dt) - shift) / scale for im in (img1, img2)]
        for layer in ARCH[net]:
            if layer[0] == "conv":
                _, _, _, _, stride, pad, key = layer
                w = torch.from_numpy(weights[key + ".weight"]).to(dt)
                b = torch.from_numpy(weights[key + ".bias"]).to(dt)
                xs = [F.relu(F.conv2d(x, w, b, stride=stride, padding=pad)) for x in xs]
            elif layer[0] == "pool":
                xs = [F.max_pool2d(x, kernel_size=layer[1], stride=layer[2]) for x in xs]
            else:
                lin = torch.from_numpy(weights[f"lin{layer[1]}.model.1.weight"]).to(dt)
                f0, f1 = [x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10) for x in xs]
                maps.append(F.conv2d((f0 - f1) ** 2, lin)[0, 0].double().numpy().copy())
    return maps


def tap_strides(net: str) -> List[int]:
    """Cumulative stride of the five tapped activations against the input (vgg: 1, 2, 4, 8, 16; alex: 4, 8, 16, 16, 16)."""
    s, out = 1, []
    for layer in ARCH[net]:
        if layer[0] == "conv":
            s *= layer[4]
        elif layer[0] == "pool":
            s *= layer[2]
        else:
            out.append(s)
    return out


def tile_grid(h: int, w: int, tile: int) -> Tuple[int, int]:
    """(tiles_y, tiles_x) of the row-major tile grid; tile <= 0 is one tile."""
    if tile <= 0:
        return 1, 1
    return -(-h // tile), -(-w // tile)


def owned(ext: int, stride: int, tile: int, t: int, ntiles: int) -> Tuple[int, int]:
    """[a, b) of a tap's axis of extent ext that tile t of ntiles owns: [min(t T // S, ext), min((t + 1) T // S, ext)), the last
    tile to the end."""
    if ntiles == 1:
        return 0, ext
    a = min(t * tile // stride, ext)
    b = ext if t == ntiles - 1 else min((t + 1) * tile // stride, ext)
    return a, max(a, b)


def cell(m: np.ndarray, stride: int, tile: int, ty: int, tx: int, tiles_y: int, tiles_x: int):
    """The part of map m that tile (ty, tx) owns (a view; empty where the tile owns nothing of this tap)."""
    ya, yb = owned(m.shape[0], stride, tile, ty, tiles_y)
    xa, xb = owned(m.shape[1], stride, tile, tx, tiles_x)
    return m[ya:yb, xa:xb]


def cell_sums(maps: List[np.ndarray], net: str, h: int, w: int, tile: int) -> np.ndarray:
    """(tiles, 5) float64: per tile of the row-major grid and per tap the sum of the map over the cell the tile owns."""
    tiles_y, tiles_x = tile_grid(h, w, tile)
    strides = tap_strides(net)
    out = np.zeros((tiles_y * tiles_x, 5))
    for t in range(tiles_y * tiles_x):
        for k in range(5):
            out[t, k] = cell(maps[k], strides[k], tile, t // tiles_x, t % tiles_x, tiles_y, tiles_x).sum()
    return out


def cell_sizes(net: str, h: int, w: int, tile: int) -> np.ndarray:
    """(tiles, 5) int: pixels of each tap a tile owns (0: the tile contributes nothing there)."""
    tiles_y, tiles_x = tile_grid(h, w, tile)
    strides = tap_strides(net)
    sizes = lo.layer_sizes(net, h, w)
    out = np.zeros((tiles_y * tiles_x, 5), dtype=np.int64)
    for t in range(tiles_y * tiles_x):
        for k in range(5):
            ya, yb = owned(sizes[k][0], strides[k], tile, t // tiles_x, tiles_y)
            xa, xb = owned(sizes[k][1], strides[k], tile, t % tiles_x, tiles_x)
            out[t, k] = (yb - ya) * (xb - xa)
    return out
