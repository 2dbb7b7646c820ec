"""NumPy restatement of the geometric self-ensemble of include/sr_hip.h: the eight transforms T_k, their inverses, and the
ensemble of a forward over the members of a mask.  Nothing here touches the library."""
from __future__ import annotations

import numpy as np


def d4(x: np.ndarray, k: int) -> np.ndarray:
    """T_k(x) on an H x W x C array: if k & 1 a horizontal flip, then if k & 2 a vertical flip, then if k & 4 a transpose of
    the two spatial axes (W x H x C)."""
    assert 0 <= k <= 7 and x.ndim == 3
    if k & 1:
        x = x[:, ::-1]
    if k & 2:
        x = x[::-1]
    if k & 4:
        x = x.transpose(1, 0, 2)
    return np.ascontiguousarray(x)


def d4_inv(y: np.ndarray, k: int) -> np.ndarray:
    """T_k^-1(y): the three steps undone in reverse order."""
    assert 0 <= k <= 7 and y.ndim == 3
    if k & 4:
        y = y.transpose(1, 0, 2)
    if k & 2:
        y = y[::-1]
    if k & 1:
        y = y[:, ::-1]
    return np.ascontiguousarray(y)


def members(mask: int):
    assert 1 <= mask <= 255
    return [k for k in range(8) if mask >> k & 1]


def mean_f32(ys) -> np.ndarray:
    """s = y_1; s = s + y_2; ...; o = s / (float)n, every step in np.float32."""
    s = np.asarray(ys[0], dtype=np.float32).copy()
    for y in ys[1:]:
        s = (s + np.asarray(y, dtype=np.float32)).astype(np.float32)
    return (s / np.float32(len(ys))).astype(np.float32)


def ensemble(forward, x: np.ndarray, mask: int) -> np.ndarray:
    """o of the definition: forward(u8 H x W x 3) -> fp32 (H s) x (W s) x 3; members ascending."""
    return mean_f32([d4_inv(forward(d4(x, k)), k) for k in members(mask)])


def to_u8(o: np.ndarray) -> np.ndarray:
    """rintf(fminf(fmaxf(o, 0), 1) * 255) in fp32."""
    o = np.asarray(o, dtype=np.float32)
    return np.rint(np.clip(o, np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)


def row_stride(row_bytes: int) -> int:
    return (row_bytes + 15) // 16 * 16


def workspace_bytes(h: int, w: int, scale: int, mask: int) -> int:
    """sr_ens_plan's workspace, restated from the header: accumulator + one forward output + transformed u8 input, row strides
    rounded up to 16 bytes, sections to 256."""
    def sect(rows, row_bytes):
        return (rows * row_stride(row_bytes) + 255) // 256 * 256
    H, W = h * scale, w * scale
    plain, transposing = bool(mask & 0x0F), bool(mask & 0xF0)
    acc = sect(H, W * 12)
    y = max(sect(H, W * 12) if plain else 0, sect(W, H * 12) if transposing else 0)
    inp = max(sect(h, w * 3) if mask & 0x0E else 0, sect(w, h * 3) if transposing else 0)
    return acc + y + inp
