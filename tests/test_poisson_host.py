"""Host side of Poisson fusion and seam repair (no GPU): the C ABI exports, the soundness of the restatement
(tests/_poisson_ref.py) without OpenCV, and BlendingModule's rectangle / fallback / ordering logic that runs before any
device call."""
import numpy as np
import pytest
from scipy import fft as sfft
from scipy import ndimage as ndi

import _native
import _poisson_ref as R
import blending_module as bm


def test_library_exports_the_poisson_entry_points():
    lib = _native.load()
    for name in ("sr_poisson_clone_u8", "sr_poisson_max_side", "sr_gaussian_blur15_u8", "sr_region_ssim_u8",
                 "sr_resize_linear_u8"):
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES
    assert _native.POISSON_MAX_SIDE == lib.sr_poisson_max_side() == lib.sr_fft_max_len() // 2 + 1 == 16385


# ---- the restatement is sound ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [R.NORMAL, R.MIXED, R.MONOCHROME])
def test_solution_satisfies_the_discrete_poisson_equation(mode):
    dest, patch, mask = R.solver_inputs(61, 83)
    _, r = R.clone(dest, patch, mask, mode, np.float64, raw=True)
    _, lap = R.guidance(dest, patch, mask, mode, np.float64)
    full = dest.astype(np.float64)
    full[1:-1, 1:-1] = r
    five = full[1:-1, :-2] + full[1:-1, 2:] + full[:-2, 1:-1] + full[2:, 1:-1] - 4 * full[1:-1, 1:-1]
    assert np.abs(five - lap).max() <= 1e-8 * np.abs(lap).max()


def test_dst1_by_odd_extension_equals_scipy():
    x = np.random.default_rng(3).normal(size=(5, 130))
    want = sfft.dst(x, type=1, axis=-1)
    assert np.abs(R.dst1_by_fft(x) - want).max() <= 1e-11 * np.abs(want).max()


@pytest.mark.parametrize("mode", [R.NORMAL, R.MIXED, R.MONOCHROME])
def test_cloning_the_destination_onto_itself_changes_nothing(mode):
    dest, _, mask = R.solver_inputs(64, 96)
    if mode == R.MONOCHROME:                      # the gray patch of a gray destination is the destination
        dest = np.repeat(R.rgb2gray(dest)[..., None], 3, axis=2)
    for dt in (np.float64, np.float32):
        assert np.array_equal(R.clone(dest, dest, mask, mode, dt), dest)


def test_blur_restatement_against_scipy():
    assert int(R.BLUR15_TAPS.sum()) == 256 and np.array_equal(R.BLUR15_TAPS, R.BLUR15_TAPS[::-1])
    for shape in ((90, 120, 3), (40, 33), (9, 50, 4)):
        img = R.synth(shape[0], shape[1], 5)
        img = img[..., 0] if len(shape) == 2 else np.concatenate([img, img[..., :1]], 2)[..., :shape[2]]
        want = ndi.gaussian_filter(img.astype(np.float64), sigma=(2.6, 2.6) + (0,) * (img.ndim - 2), truncate=7 / 2.6,
                                   mode="mirror")
        got = R.gaussian_blur15(img)
        assert got.dtype == np.uint8 and got.shape == img.shape
        assert np.abs(got.astype(np.float64) - want).max() <= 1.0


# ---- host logic of the mirror ------------------------------------------------------------------------------------------
def _mask(h, w, box):
    m = np.zeros((h, w), np.uint8)
    x0, y0, x1, y1 = box
    m[y0:y1, x0:x1] = 255
    return m


@pytest.mark.parametrize("box,center,dst_hw,want", [
    ((10, 8, 30, 20), (50, 40), (80, 100), ((10, 8, 20, 12), (40, 34, 20, 12))),
    ((0, 0, 40, 30), (50, 40), (80, 100), ((1, 1, 38, 28), (31, 26, 38, 28))),        # mask touching the frame loses it
    ((5, 5, 26, 16), (3, 40), (80, 100), None),                                     # roi_d leaves the destination
    ((5, 5, 26, 16), (95, 75), (80, 100), None),
    ((0, 0, 40, 1), (50, 40), (80, 100), None),                                     # only frame pixels: nothing left
])
def test_clone_rectangles(box, center, dst_hw, want):
    m = _mask(30, 40, box)
    got = bm.BlendingModule._clone_rects(m.copy(), dst_hw, center)
    assert got == want
    assert R.clone_rects(m.copy(), dst_hw, center) == want


def test_fallback_decisions_need_no_device():
    b = bm.BlendingModule()
    rng = np.random.default_rng(11)
    dst = rng.integers(0, 256, (60, 80, 3), dtype=np.uint8)
    src = rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)
    # all-zero mask: dst back unchanged (a copy)
    out = b.poisson_fusion(src, dst, np.zeros((30, 40), np.uint8))
    assert np.array_equal(out, dst) and out is not dst
    # gray inputs, roi_d outside, float mask with nothing inside its frame: the reference's host blend, byte for byte
    gray_s, gray_d = src[..., 0], dst[..., 0]
    m = _mask(30, 40, (4, 4, 30, 20))
    cases = [(gray_s, gray_d, m, None), (src, dst, m, (5, 5)), (src, dst, _mask(30, 40, (0, 0, 40, 1)).astype(np.float32), None),
             (src.astype(np.float32) * 1.5 - 20, dst.astype(np.float64), m, (78, 58))]
    for s, d, mk, c in cases:
        assert np.array_equal(b.poisson_fusion(s, d, mk, c), R.poisson_fusion(s, d, mk, c))
    # mask of another shape than src: what the host blend itself does with it (the reference's behaviour)
    big = _mask(50, 60, (5, 5, 40, 30))
    assert np.array_equal(b.poisson_fusion(src, dst, big), R.poisson_fusion(src, dst, big))


def test_refusals_before_any_device_call():
    b = bm.BlendingModule()
    with pytest.raises(NotImplementedError):
        b.poisson_fusion(None, None)
    with pytest.raises(NotImplementedError):
        b.poisson_fusion([[1]], np.zeros((4, 4, 3), np.uint8))
    # a clone rectangle above the side limit: refused on the host (tiny dtype-less views keep this test cheap)
    n = _native.POISSON_MAX_SIDE + 3
    src = np.broadcast_to(np.zeros((1, 1, 3), np.uint8), (4, n, 3))
    dst = np.broadcast_to(np.zeros((1, 1, 3), np.uint8), (4, n, 3))
    with pytest.raises(NotImplementedError, match="side limit"):
        b.poisson_fusion(src, dst)
    ctx_free = _native.Context.__new__(_native.Context)           # no device behind it: the check must come first
    with pytest.raises(NotImplementedError):
        _native.Context.poisson_clone_u8(ctx_free, 0, 0, 0, 0, 0, 0, 5, n, 1, 0, 0)
    with pytest.raises(NotImplementedError):
        b.repair_seams(np.zeros((8, 8, 3), np.float32), [bm.Seam(1, 1, 2, 2, 0.5)], [])
    with pytest.raises(NotImplementedError):
        b.repair_seams(np.zeros((8, 8), np.uint8), [bm.Seam(1, 1, 2, 2, 0.5)], [])


def test_repair_seams_methods_that_change_nothing():
    b = bm.BlendingModule()
    img = R.synth(40, 50, 3)
    seams = [bm.Seam(4, 4, 16, 16, 0.5), bm.Seam(20, 10, 16, 16, 0.9), bm.Seam(0, 0, 16, 16, 0.99)]
    for method in ("blend", "poisson", "none"):
        out = b.repair_seams(img, seams, [img], method)
        assert np.array_equal(out, img) and out is not img
        assert np.array_equal(R.repair_seams(img, seams, [img], method), img)
    assert np.array_equal(b.repair_seams(img, seams[2:], [img]), img)          # "auto" with only low-severity seams
    assert np.array_equal(b.repair_seams(img, [], [img]), img)


def test_restated_repair_is_ordered():
    """Overlapping blur seams: the second box reads what the first wrote, so the order matters in the restatement the GPU
    test compares against."""
    img = R.synth(80, 100, 4)
    a, c = bm.Seam(20, 20, 16, 16, 0.9), bm.Seam(36, 28, 16, 16, 0.9)
    ab, ba = R.repair_seams(img, [a, c], [img]), R.repair_seams(img, [c, a], [img])
    assert not np.array_equal(ab, ba)
    first = img.copy()
    xa, ya, xb, yb = R.padded_box(a, img.shape)
    first[ya:yb, xa:xb] = R.gaussian_blur15(img[ya:yb, xa:xb])
    xa, ya, xb, yb = R.padded_box(c, img.shape)
    first[ya:yb, xa:xb] = R.gaussian_blur15(first[ya:yb, xa:xb])
    assert np.array_equal(ab, first)
