"""GPU: BlendingModule.gradient_domain_fusion and compute_blend_quality (csrc/sr_gradient.hip) against the NumPy restatement
in tests/_gradient_ref.py.  Bar: the u8 canvas is byte-equal for integer-valued tiles (u8, u16, whole-number float32) and
for non-integer float32 tiles in the restated Sobel order; the SSIM fields of compute_blend_quality match to 1e-12, the
gradient fields the float64 restatement to 1e-9 relative and the reference's float32 expressions to 1e-5."""
import numpy as np
import pytest

import _gradient_ref as gref
import blending_module as bm

pytestmark = pytest.mark.gpu


def _tiles(rng, n, h, w, cn=3, dtype=np.uint8):
    """Disagreeing tiles: a per-tile offset plus seeded noise (as test_gpu_blend.py builds them)."""
    out = []
    for i in range(n):
        yy, xx = np.mgrid[0:h, 0:w]
        base = 128 + 64 * np.sin(xx / 37.0 + i) + 48 * np.cos(yy / 23.0 + 0.5 * i)
        img = np.clip(base[..., None] + rng.integers(-12, 13, (h, w, cn)) + 7 * i, 0, 255)
        out.append(img.astype(dtype) if cn > 1 else img[..., 0].astype(dtype))
    return out


def _grid(th, tw, ov, rows, cols):
    return [(r * (th - ov), c * (tw - ov)) for r in range(rows) for c in range(cols)]


def _check(tiles, pos, shape):
    got = bm.BlendingModule().gradient_domain_fusion(tiles, pos, shape)
    want = gref.gradient_domain_fusion(tiles, pos, shape)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} bytes differ"
    return got


@pytest.mark.parametrize("cn", [3, 1])
def test_grid_u8(rng, cn):
    pos = _grid(60, 80, 16, 3, 3)
    _check(_tiles(rng, 9, 60, 80, cn), pos, (60 * 3 - 32, 80 * 3 - 32))


def test_u16_and_whole_number_float_tiles(rng):
    pos = _grid(48, 64, 12, 2, 2)
    u16 = [(t.astype(np.uint16) * 3 + 100).astype(np.uint16) for t in _tiles(rng, 4, 48, 64)]
    _check(u16, pos, (84, 116))                            # values past 255: the canvas saturates, as the reference's
    _check([t.astype(np.float32) for t in _tiles(rng, 4, 48, 64)], pos, (84, 116))
    _check([t.astype(np.int32) for t in _tiles(rng, 4, 48, 64, 1)], pos, (84, 116))


def test_non_integer_float_tiles(rng):
    pos = _grid(40, 52, 10, 2, 3)
    tiles = [(t.astype(np.float32) * np.float32(0.731) + np.float32(0.3)) for t in _tiles(rng, 6, 40, 52)]
    _check(tiles, pos, (70, 136))                          # OpenCV's own summation order: parity unpinned


def test_clipped_gaps_odd_sizes_and_thin_strips(rng):
    # a tile running past the right and bottom edges, an uncovered gap, odd sizes, RGBA
    tiles = _tiles(rng, 3, 37, 41, 4)
    _check(tiles, [(0, 0), (0, 50), (30, 20)], (53, 77))
    # tiles that reach the canvas as 2-pixel-thin strips (the Sobel still sees their rows outside the canvas)
    t = _tiles(rng, 3, 16, 24)
    _check(t, [(0, 0), (0, 22), (14, 5)], (16, 24))
    # a 2-row canvas
    _check(_tiles(rng, 2, 9, 30), [(0, 0), (1, 20)], (2, 45))


def test_example_compare_methods_grid(rng):
    """The 2 x 2 grid of the reference's example_compare_methods (:2062-2139): 256 px tiles, 32 px overlap."""
    tiles = _tiles(rng, 4, 256, 256)
    pos = [(0, 0), (0, 224), (224, 0), (224, 224)]
    _check(tiles, pos, (480, 480))


def test_long_chains(rng):
    """Full-length lines of the 200 MP grid: a 17320-wide row chain and an 11550-tall column chain."""
    tiles = _tiles(rng, 5, 20, 3600)
    _check(tiles, [(0, c * 3430) for c in range(5)], (20, 17320))
    tall = _tiles(rng, 4, 2950, 16, 1)
    _check(tall, [(r * 2866, 0) for r in range(4)], (11550, 16))


def _quality_case(rng):
    tiles = _tiles(rng, 4, 64, 80)
    pos = [(0, 0), (0, 64), (48, 0), (48, 64)]
    shape = (100, 130)                                    # the right-hand tiles are clipped by the canvas (80 -> 66 wide)
    return tiles, pos, shape


def _quality_check(result, tiles, pos):
    got = bm.compute_blend_quality(result, tiles, pos)
    want = gref.compute_blend_quality(result, tiles, pos)
    lit = gref.compute_blend_quality(result, tiles, pos, literal=True)
    for k in ("mean_ssim", "min_ssim", "std_ssim"):
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
    for k in ("mean_gradient", "gradient_discontinuity"):
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), (k, got[k], want[k])
        assert abs(got[k] - lit[k]) <= 1e-5 * abs(lit[k]), (k, got[k], lit[k])


@pytest.mark.parametrize("method", ["laplacian", "weighted", "feather", "gradient"])
def test_compute_blend_quality(rng, method):
    tiles, pos, shape = _quality_case(rng)
    m = bm.BlendingModule()
    infos = [bm.TileInfo(t, x, y, t.shape[1], t.shape[0]) for t, (y, x) in zip(tiles, pos)]
    if method == "laplacian":
        result = m.laplacian_fusion(infos, output_shape=shape)
    elif method == "weighted":
        result = m.weighted_average_fusion(infos, output_shape=shape)
    elif method == "feather":
        result = m.feather_blend(infos, output_shape=shape)
    else:
        result = m.gradient_domain_fusion(tiles, pos, shape)
    _quality_check(result, tiles, pos)


def test_compute_blend_quality_gray_and_rgba(rng):
    tiles = _tiles(rng, 2, 40, 50, 1)
    pos = [(0, 0), (10, 30)]
    result = bm.BlendingModule().gradient_domain_fusion(tiles, pos, (45, 70))
    _quality_check(result, tiles, pos)
    tiles = _tiles(rng, 2, 40, 50, 4)
    result = bm.BlendingModule().gradient_domain_fusion(tiles, pos, (45, 70))
    _quality_check(result, tiles, pos)
