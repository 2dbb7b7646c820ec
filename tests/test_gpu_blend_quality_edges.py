"""GPU: the reductions behind compute_blend_quality (csrc/sr_gradient.hip: k_grad_mag, k_tile_ssim) at the shapes where their
loops and their launch shape change.

  sr_gradient_stats_u8   one-pixel, one-row and one-column images (refl(.., 1)), 300 rows (the row loop y += gridDim.y runs
                         twice: the grid has at most 256 rows of blocks), 2100 and 3 x 700 row elements (the element loop runs
                         twice: 8 blocks of 256 threads per row), every channel count 1..4 (k_grad_mag<2> has no other caller),
                         a padded row stride.  The sum of squares is an exact integer; the magnitude sum is held to the
                         recursive-summation bound N * 2^-53 relative (N elements, all terms positive, every square root
                         correctly rounded on both sides, so only the order of the additions differs) against math.fsum.
  sr_tile_ssim_sums_u8   one call holding a 300 x 1100 tile (ROI above the 256 x 1024 the grid covers in one step: both loops of
                         the kernel run twice), a 1 x 1 and a 9 x 9 tile (the grid is sized from the largest tile, so most of
                         their blocks have nothing to add) and a tile clipped by the right and bottom canvas edges (the resize
                         branch), for cn 1, 3, 4 and both gray conversions: the five sums are exact integers."""
import math

import numpy as np
import pytest

import _gradient_ref as gref
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu


def _stats_ref(img):
    a = img if img.ndim == 3 else img[..., None]
    sq = []
    for c in range(a.shape[2]):
        gx, gy = gref.sobel_f32(a[:, :, c])                      # integer-valued (|g| <= 1020): exact in float32
        gx, gy = gx.astype(np.int64), gy.astype(np.int64)
        sq.append(gx * gx + gy * gy)
    sq = np.stack(sq, axis=-1)
    return int(sq.sum()), math.fsum(np.sqrt(sq.astype(np.float64)).ravel().tolist())


def _stats_check(ctx, img, stride=None):
    h, w = img.shape[:2]
    cn = img.shape[2] if img.ndim == 3 else 1
    want_sq, want_mag = _stats_ref(img)
    if stride is None:
        buf, stride = ctx.upload(img), w * cn
    else:
        padded = np.full((h, stride), 0xEE, np.uint8)
        padded[:, :w * cn] = img.reshape(h, w * cn)
        buf = ctx.upload(padded)
    try:
        sq, mag = ctx.gradient_stats_u8(buf.ptr, stride, h, w, cn)
    finally:
        buf.free()
    print(f"gradient_stats {h}x{w}x{cn}: sq {sq} (want {want_sq}), mag {mag!r} (want {want_mag!r}, "
          f"rel {abs(mag - want_mag) / max(want_mag, 1e-300):.3e}, bound {h * w * cn * 2.0 ** -53:.3e})")
    assert sq == want_sq
    assert abs(mag - want_mag) <= h * w * cn * 2.0 ** -53 * want_mag


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (2, 2), (300, 40), (3, 2100), (5, 700, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_gradient_stats_loop_and_border_shapes(ctx, rng, shape):
    _stats_check(ctx, rng.integers(0, 256, shape).astype(np.uint8))


@pytest.mark.parametrize("cn", [1, 2, 3, 4])
def test_gradient_stats_every_channel_count(ctx, rng, cn):
    _stats_check(ctx, rng.integers(0, 256, (37, 53, cn)).astype(np.uint8))


def test_gradient_stats_padded_stride(ctx, rng):
    _stats_check(ctx, rng.integers(0, 256, (37, 53, 3)).astype(np.uint8), stride=53 * 3 + 29)


def _gray(img, shift):
    return (onp.bgr2gray_on_rgb_u8(img[..., :3], shift) if img.ndim == 3 else img).astype(np.int64)


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_tile_ssim_sums_large_tiny_and_clipped_tiles(ctx, rng, cn):
    H, W = 320, 1200
    shape = lambda h, w: (h, w) if cn == 1 else (h, w, cn)       # noqa: E731
    canvas = rng.integers(0, 256, shape(H, W)).astype(np.uint8)
    rects = [(10, 5, 1100, 300), (1150, 3, 1, 1), (20, 310, 9, 9), (W - 50, H - 70, 90, 120)]      # (x, y, w, h)
    tiles = [rng.integers(0, 256, shape(h, w)).astype(np.uint8) for (_, _, w, h) in rects]
    assert rects[0][3] > 256 and rects[0][2] > 1024 and rects[3][0] + rects[3][2] > W and rects[3][1] + rects[3][3] > H
    dc, dts = ctx.upload(canvas), [ctx.upload(t) for t in tiles]
    try:
        for shift in (15, 14):
            got = ctx.tile_ssim_sums_u8(dc.ptr, W * cn, H, W, cn, rects, [d.ptr for d in dts], [r[2] * cn for r in rects], shift)
            assert got.shape == (4, 5)
            for t, (x, y, w, h) in enumerate(rects):
                roi = canvas[y:y + h, x:x + w]
                tile = tiles[t]
                if roi.shape != tile.shape:                      # compute_blend_quality: cv2.resize(tile, (roi_w, roi_h))
                    tile = gref._resize_u8(tile, roi.shape[1], roi.shape[0])
                a, b = _gray(roi, shift), _gray(tile, shift)
                want = [int(a.sum()), int(b.sum()), int((a * a).sum()), int((b * b).sum()), int((a * b).sum())]
                assert [int(v) for v in got[t]] == want, (cn, shift, t)
    finally:
        for d in [dc] + dts:
            d.free()
