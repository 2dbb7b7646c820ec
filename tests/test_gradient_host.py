"""CPU: the NumPy restatement of gradient_domain_fusion / compute_blend_quality (tests/_gradient_ref.py) against SciPy's
Sobel and against explicit fp32 loops, and the argument checks both functions make before any device call."""
import numpy as np
import pytest
from scipy import ndimage

import _gradient_ref as gref
import blending_module as bm


def _int_tiles(rng, n, h, w, cn=3):
    out = []
    for i in range(n):
        yy, xx = np.mgrid[0:h, 0:w]
        base = 128 + 64 * np.sin(xx / 7.0 + i) + 48 * np.cos(yy / 5.0 + 0.5 * i)
        img = np.clip(base[..., None] + rng.integers(-12, 13, (h, w, cn)) + 9 * i, 0, 255).astype(np.uint8)
        out.append(img if cn > 1 else img[..., 0])
    return out


def test_sobel_matches_scipy_on_integer_data():
    rng = np.random.default_rng(3)
    for shape in [(9, 13), (16, 8), (3, 40), (31, 2)]:
        a = rng.integers(0, 256, shape).astype(np.float32)
        gx, gy = gref.sobel_f32(a)
        assert gx.dtype == np.float32 and gy.dtype == np.float32
        assert np.array_equal(gx, ndimage.sobel(a.astype(np.float64), axis=1, mode="mirror"))
        assert np.array_equal(gy, ndimage.sobel(a.astype(np.float64), axis=0, mode="mirror"))


def test_weight_map_is_the_modules():
    m = bm.BlendingModule()
    for h, w in [(8, 8), (40, 17), (64, 100)]:
        assert np.array_equal(gref.weight_map(h, w), m._create_distance_weight_map(h, w, bm.WeightType.COSINE))


@pytest.mark.parametrize("cn", [1, 3])
def test_restatement_equals_explicit_loops(cn):
    rng = np.random.default_rng(11 + cn)
    tiles = _int_tiles(rng, 4, 12, 14, cn)
    pos = [(0, 0), (0, 9), (7, 0), (7, 9)]             # overlaps, and the last two tiles run past the canvas
    out = gref.gradient_domain_fusion(tiles, pos, (17, 21))
    assert np.array_equal(out, gref.gradient_domain_fusion_loops(tiles, pos, (17, 21)))
    # non-integer float data and an uncovered gap
    ftiles = [t.astype(np.float32) * np.float32(0.37) + np.float32(0.11) for t in tiles[:2]]
    fpos = [(0, 0), (5, 12)]
    assert np.array_equal(gref.gradient_domain_fusion(ftiles, fpos, (18, 27)),
                          gref.gradient_domain_fusion_loops(ftiles, fpos, (18, 27)))


def test_cumsum_is_a_sequential_fp32_chain():
    v = np.random.default_rng(2).uniform(-3, 3, 5000).astype(np.float32)
    run, seq = np.float32(0), np.empty_like(v)
    for i, x in enumerate(v):
        run = np.float32(run + x)
        seq[i] = run
    assert np.array_equal(np.cumsum(v), seq)


def test_quality_restatement_literal_and_float64_agree():
    rng = np.random.default_rng(5)
    tiles = _int_tiles(rng, 4, 20, 24)
    pos = [(0, 0), (0, 18), (14, 0), (14, 18)]
    canvas = gref.gradient_domain_fusion(tiles, pos, (30, 36))
    a = gref.compute_blend_quality(canvas, tiles, pos)
    b = gref.compute_blend_quality(canvas, tiles, pos, literal=True)
    for k in ("mean_ssim", "min_ssim", "std_ssim"):
        assert a[k] == b[k]
    for k in ("mean_gradient", "gradient_discontinuity"):
        assert abs(a[k] - b[k]) <= 1e-5 * abs(a[k])


def test_compute_blend_quality_is_importable():
    from blending_module import compute_blend_quality   # noqa: F401
    assert callable(bm.compute_blend_quality)


def test_gradient_domain_fusion_refuses_bad_arguments_without_a_gpu():
    m = bm.BlendingModule()
    rgb = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(ValueError):
        m.gradient_domain_fusion([rgb, np.zeros((16, 16), np.uint8)], [(0, 0), (0, 8)], (32, 32))     # mixed ndim
    with pytest.raises(ValueError):
        m.gradient_domain_fusion([rgb, np.zeros((16, 16, 4), np.uint8)], [(0, 0), (0, 8)], (32, 32))  # channel count
    for bad in [(-1, 0), (0, -3), (32, 0), (0, 40)]:
        with pytest.raises(ValueError):
            m.gradient_domain_fusion([rgb], [bad], (32, 40))
    with pytest.raises(ValueError):
        m.gradient_domain_fusion([np.zeros((7, 30, 3), np.uint8)], [(0, 0)], (32, 32))                # zero feather width
    with pytest.raises(ValueError):
        m.gradient_domain_fusion([], [], (32, 32))
    with pytest.raises(NotImplementedError):
        m.gradient_domain_fusion([np.zeros((16, 16, 5), np.uint8)], [(0, 0)], (32, 32))


def test_compute_blend_quality_refuses_bad_arguments_without_a_gpu():
    canvas = np.zeros((32, 32, 3), np.uint8)
    t = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(NotImplementedError):
        bm.compute_blend_quality(canvas.astype(np.float32), [t], [(0, 0)])
    with pytest.raises(NotImplementedError):
        bm.compute_blend_quality(canvas, [t.astype(np.uint16)], [(0, 0)])
    with pytest.raises(ValueError):
        bm.compute_blend_quality(canvas, [t, t[..., 0]], [(0, 0), (8, 8)])
    with pytest.raises(ValueError):
        bm.compute_blend_quality(canvas, [t[..., 0]], [(0, 0)])                # gray tile on an RGB canvas
    with pytest.raises(ValueError):
        bm.compute_blend_quality(canvas, [t], [(32, 0)])
    with pytest.raises(ValueError):
        bm.compute_blend_quality(canvas[..., :2], [t[..., :2]], [(0, 0)])     # BGR2GRAY needs 3 or 4 channels
