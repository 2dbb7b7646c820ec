"""GPU: ContentAnalyzer's HIP kernels (csrc/sr_content.hip) against the NumPy restatement of the reference
(tests/_content_ref.py), and the roi_flags split_array fills from them.

Saliency bounds: every pixel within 1 grey level of the float64 restatement (a condition); the share of pixels that
differ at all is held to 8x the share the same restatement shows when evaluated in complex64 NumPy on the same input
(the GPU's FFT mixes radices and Bluestein with fp32 twiddles and orders the 25-term mean differently), with a floor of 16
pixels so that a tiny image cannot fail on one pixel.
Entropy bound: H <= 8 bits from 256 terms, fp32 epsilon 6e-8, pairwise sum + log2 error about 5e-6, x4 for the different
summation order -> 2e-5 absolute against the float32 restatement."""
import numpy as np
import pytest

import _content_ref as R
import tiling_module as tm

pytestmark = pytest.mark.gpu

THR = int(255 * 0.7)


@pytest.fixture(scope="module")
def ca(ctx):
    return tm.ContentAnalyzer()


@pytest.mark.parametrize("h,w,cn", R.SALIENCY_CASES)
def test_saliency_matches_restatement(ca, h, w, cn):
    img = R.synthetic(h, w, cn)
    want = R.saliency(img)
    assert R.min_spectrum_magnitude(img) > 1.0                       # the fixture is not degenerate ...
    assert int((want > THR).sum()) >= 1                              # ... and has a salient spot
    got = ca.compute_saliency_map(img)
    assert got.dtype == np.uint8 and got.shape == (h, w)
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    c64 = R.saliency(img, np.float32)
    share64 = float(np.mean(c64 != want))
    n_diff = int(np.count_nonzero(diff))
    allowed = max(8.0 * share64 * diff.size, 16.0)
    print(f"saliency {h}x{w}x{cn}: max |diff| {int(diff.max())}, differing {n_diff} px (share {n_diff / diff.size:.3g}), "
          f"complex64 NumPy share {share64:.3g}, allowed {allowed:.1f} px")
    assert int(diff.max()) <= 1
    assert n_diff <= allowed
    assert np.array_equal(ca.compute_saliency_map(img), got)         # two calls, identical bytes


def test_saliency_of_a_constant_image_is_finite_u8(ca):
    for shape in ((48, 80, 3), (33, 33), (1, 1, 3), (2, 3)):
        got = ca.compute_saliency_map(np.full(shape, 77, np.uint8))
        assert got.dtype == np.uint8 and got.shape == shape[:2]


@pytest.mark.parametrize("win", [1, 7, 64, 256])
@pytest.mark.parametrize("h,w,cn", [(150, 201, 3), (300, 520, 1), (40, 50, 4)])
def test_local_entropy_matches_restatement(ca, h, w, cn, win):
    img = R.synthetic(h, w, cn, seed=21)
    want = R.local_entropy(img, win)
    got = ca.compute_local_entropy(img, win)
    assert got.dtype == np.float32 and got.shape == (h, w)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"entropy {h}x{w}x{cn} window {win}: max |diff| {err:.3g}")
    assert err <= 2e-5
    for y in range(0, h, win):
        for x in range(0, w, win):
            cell = got[y:y + win, x:x + win]
            assert np.all(cell == cell[0, 0])                        # exactly constant within a cell


def test_local_entropy_default_window_and_flat_cells(ca):
    img = np.zeros((100, 130, 3), np.uint8)
    img[:, 64:] = R.synthetic(100, 66, 3, seed=2)
    got = ca.compute_local_entropy(img)
    assert np.array_equal(got, ca.compute_local_entropy(img, 64))
    assert np.all(np.abs(got[:64, :64]) <= 2e-5)                      # one grey level: H = -1 log2(1 + 1e-10)
    assert np.abs(got - R.local_entropy(img, 64)).max() <= 2e-5


def _stub(boxes):
    return lambda image: list(boxes)


@pytest.mark.parametrize("h,w,cn", [(257, 384, 3), (120, 200, 1), (255, 301, 3)])
def test_forbidden_map_matches_restatement(h, w, cn):
    img = R.synthetic(h, w, cn)
    faces = [(w - 30, h - 20, 50, 40), (5, 8, 21, 33), (w // 2, h // 2, 10, 10)]       # one overflows, one clips at 0
    texts = [(w - 10, 3, 40, 25), (0, h - 4, 17, 30), (w + 5, 2, 4, 4), (12, 40, 0, 9)]  # overflow, outside, empty
    an = tm.ContentAnalyzer(face_detector=_stub(faces), text_detector=_stub(texts))
    sal = R.saliency(img)
    # rectangles alone are exact
    rect_only = an.create_forbidden_zone_map(img, protect_salient=False)
    assert rect_only.dtype == bool and np.array_equal(rect_only, R.forbidden_map(img, faces, texts, protect_salient=False))
    # with saliency: equal everywhere except where the restatement's saliency is within 1 of the threshold
    for thr in (0.7, 0.3):
        got = an.create_forbidden_zone_map(img, saliency_threshold=thr)
        want = R.forbidden_map(img, faces, texts, True, thr, saliency_map=sal)
        loose = np.abs(sal.astype(np.int32) - int(255 * thr)) <= 1
        assert np.array_equal(got[~loose], want[~loose])
        assert got.any() and not got.all()
    # no detectors, no text: saliency alone
    plain = tm.ContentAnalyzer().create_forbidden_zone_map(img, protect_text=False)
    loose = np.abs(sal.astype(np.int32) - THR) <= 1
    assert np.array_equal(plain[~loose], (sal > THR)[~loose])


def test_tile_flags_equal_host_counts(ctx):
    img = R.synthetic(300, 420, 3)
    an = tm.ContentAnalyzer(face_detector=_stub([(100, 120, 60, 40)]))
    d_img = ctx.upload(img)
    fmap = an.create_forbidden_zone_map_device(d_img.ptr, img.shape, protect_text=False, host_image=img)
    try:
        host = fmap.download()
        assert host[120:160, 100:160].all()
        positions = [(0, 0, 180, 250), (240, 0, 180, 250), (0, 50, 180, 250), (400, 280, 180, 250), (0, 0, 420, 300),
                     (7, 3, 1, 1), (0, 290, 10, 10)]                                    # two of them clipped by the image edge
        got = an.tile_flags(fmap, positions)
        want = R.tile_flags(host, positions)
        assert got == want
        for g in got:
            assert isinstance(g['has_forbidden_zone'], bool) and isinstance(g['forbidden_ratio'], float)
        assert got[3]['forbidden_ratio'] == float(np.sum(host[280:, 400:]) / host[280:, 400:].size)
        assert any(g['has_forbidden_zone'] for g in got) and not all(g['has_forbidden_zone'] for g in got)
        with pytest.raises(ValueError):
            an.tile_flags(fmap, [(420, 0, 5, 5)])
    finally:
        fmap.free()
        d_img.free()


def _split(t, img, **kw):
    tiles = t.split_array(img, image_hash="h", save_metadata=False, **kw)
    return tiles


def test_split_array_fills_roi_flags(ctx, tmp_path):
    img = R.synthetic(300, 420, 3)
    an = tm.ContentAnalyzer(face_detector=_stub([(100, 120, 60, 40)]))
    args = {'protect_text': False}
    t = tm.TilingModule(block_size=128, overlap_ratio=0.2, l2_cache_dir=str(tmp_path), content_analyzer=an,
                        forbidden_zone_args=args)
    host_tiles = _split(t, img)
    positions = [(m.global_x, m.global_y, m.input_w, m.input_h) for m in (tl.metadata for tl in host_tiles)]
    assert any(w < 128 or h < 128 for _, _, w, h in positions)      # edge tiles: padded to the block, counted unpadded
    fm = an.create_forbidden_zone_map(img, **args)
    want = R.tile_flags(fm, positions)
    assert [tl.metadata.roi_flags for tl in host_tiles] == want
    assert any(f['has_forbidden_zone'] for f in want)
    before = (ctx.d2h_bytes, ctx.h2d_bytes)
    dev_tiles = _split(t, img, device_resident=True)
    # device-resident: the image went up once, no plane came back
    assert ctx.d2h_bytes == before[0] and ctx.h2d_bytes == before[1] + img.nbytes
    assert [tl.metadata.roi_flags for tl in dev_tiles] == want
    assert t.device_tiles.forbidden is not None
    assert np.array_equal(t.device_tiles.forbidden.download(), fm)
    t.release_device_tiles()
    assert t.device_tiles is None
    # enable_content_aware=False switches the analyzer off too
    t_off = tm.TilingModule(block_size=128, l2_cache_dir=str(tmp_path), enable_content_aware=False, content_analyzer=an,
                            forbidden_zone_args=args)
    assert all(tl.metadata.roi_flags == {} for tl in _split(t_off, img))


def test_split_array_without_analyzer_is_unchanged(ctx, tmp_path):
    img = R.synthetic(300, 420, 3)
    an = tm.ContentAnalyzer()
    plain = tm.TilingModule(block_size=128, l2_cache_dir=str(tmp_path))
    with_an = tm.TilingModule(block_size=128, l2_cache_dir=str(tmp_path), content_analyzer=an,
                              forbidden_zone_args={'protect_text': False})
    assert plain.content_analyzer is None
    a, b = _split(plain, img), _split(with_an, img)
    assert len(a) == len(b) > 1
    for ta, tb in zip(a, b):
        assert ta.metadata.roi_flags == {}
        assert np.array_equal(ta.data, tb.data)
        assert ta.metadata.complexity_score == tb.metadata.complexity_score
        ma, mb = ta.metadata, tb.metadata
        assert (ma.global_x, ma.global_y, ma.input_w, ma.input_h) == (mb.global_x, mb.global_y, mb.input_w, mb.input_h)
        # the tile bytes and the score by value: the padded extract of the source and the std of its swapped-weight gray
        x, y, w, h = ma.global_x, ma.global_y, ma.input_w, ma.input_h
        assert np.array_equal(ta.data[:h, :w], img[y:y + h, x:x + w])
        g = R.gray_bgr_rule(ta.data)
        assert ma.complexity_score == float(np.std(g))
    # device-resident without an analyzer: no map is made
    d = _split(plain, img, device_resident=True)
    assert plain.device_tiles.forbidden is None and all(tl.metadata.roi_flags == {} for tl in d)
    assert [tl.metadata.complexity_score for tl in d] == pytest.approx([tl.metadata.complexity_score for tl in a], rel=1e-12)
    plain.release_device_tiles()
