"""No GPU: the MSER definition (include/sr_hip.h, "MSER").  The Python restatement (tests/_mser_ref.py: a sorted-pixel
union-find) is held to a brute-force tree built straight from the definition through scipy.ndimage.label; the host twins of
the C ABI (sr_mser_host_u8 / sr_mser_tree_host_u8) are held to the restatement on the shapes of the GPU test; eight mutants of
the restatement are each caught by a named input; then the text-box filter at its edges, the plan and every refusal, and the
ContentAnalyzer / MserTextDetector wiring up to (not including) the first device call.  Every comparison is exact."""
import numpy as np
import pytest

import _mser_ref as R
import _native
import tiling_module as tm

CASES = R.gpu_cases()


def rows(recs):
    return [tuple(int(v) for v in r) for r in recs]


def seeded_images():
    rng = np.random.default_rng(11)
    out = []
    for i in range(24):
        h, w = (int(v) for v in rng.integers(1, 17, 2))
        levels = rng.choice(256, size=int(rng.integers(3, 13)), replace=False)
        out.append(rng.choice(levels, size=(h, w)).astype(np.uint8))
    return out


CONSTRUCTED = {k: CASES[k][0] for k in ("1x1", "1x7", "7x1", "2x2_equal", "2x2_distinct")}
CONSTRUCTED.update(diagonal=np.array([[0, 255], [255, 0]], np.uint8), steps=R.steps(10), steps6=R.steps(11),
                   checkerboard=R.checkerboard(9, 7), ramp=R.ramp()[:, :24].copy(), corridor=R.corridor(9),
                   spirals=R.spirals(13), nested=R.nested_flat()[::5, ::5].copy())


def _tree_and_regions_equal(g):
    for pol in (0, 1):
        a = 255 - g if pol else g
        assert R.trees_equal(R.tree(a), R.brute(a))
    for params in (dict(min_area=1), dict(min_area=2, max_area=40, delta=3), dict(min_area=1, delta=60, min_diversity=0.5)):
        assert R.regions(g, **params) == R.regions(g, tree_fn=R.brute, **params)


def test_restatement_equals_brute_force_on_seeded_images():
    imgs = seeded_images()
    assert len(imgs) >= 20 and all(max(g.shape) <= 16 and 1 <= len(np.unique(g)) <= 12 for g in imgs)
    for g in imgs:
        _tree_and_regions_equal(g)


@pytest.mark.parametrize("name", sorted(CONSTRUCTED))
def test_restatement_equals_brute_force_on_constructed_cases(name):
    _tree_and_regions_equal(CONSTRUCTED[name])


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twins_equal_restatement(name):
    g, params = CASES[name]
    assert rows(_native.mser_host(g, _native.mser_params(**params))) == R.regions(g, **params)
    for pol in (0, 1):
        t = _native.mser_tree_host(g, pol)
        got = np.stack([t[f].astype(np.int64) for f in t.dtype.names], axis=1)
        assert np.array_equal(got, R.node_table(R.tree(255 - g if pol else g)))


def test_host_twin_channels_masks_and_strides():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(21, 34, 4)).astype(np.uint8)
    p = _native.mser_params(min_area=2)
    for view in (img, img[..., :3], img[..., :1], img[:, :, 0], img[:, 3:29, :3], img[::2]):
        gray = R.gray_swapped(view)
        for mask in (1, 2, 3):
            assert rows(_native.mser_host(view, p, mask)) == R.regions(gray, polarity_mask=mask, min_area=2)
    assert R.gray_swapped(img[..., :3]).tolist() == R.gray_swapped(img).tolist()                   # alpha ignored


def test_expected_records_of_the_two_text_fixtures():
    text = R.regions(CASES["text"][0])
    assert len(text) == 10 and {r[0] for r in text} == {0} and len(R.tree(CASES["text"][0])["level"]) == 4721
    boxes = R.text_boxes(text, 200)
    assert sorted((w, h) for _, _, w, h in boxes) == [(22, 12)] * 5 + [(30, 20)] * 5
    nested = R.regions(CASES["nested"][0], polarity_mask=1)
    assert [r[2] for r in nested] == [384] * 4 + [8400, 12800]                                    # glyphs, panel, page
    assert [r[2] for r in R.regions(CASES["nested"][0], polarity_mask=1, mutant="strict_parent")] != [r[2] for r in nested]
    assert [r[2] for r in R.regions(CASES["nested"][0], polarity_mask=1, mutant="strict_child")] != [r[2] for r in nested]
    flat = R.regions(CASES["flat64"][0])
    assert flat == [(0, 128, 4096, 0, 0, 63, 63, 0, 4096), (1, 127, 4096, 0, 0, 63, 63, 0, 4096)] and R.text_boxes(flat, 64) == []


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_is_caught_by_its_named_input(mutant):
    name, g, params = R.mutant_inputs()[mutant]
    want = R.regions(g, **params)
    assert rows(_native.mser_host(g, _native.mser_params(**params))) == want, name                 # the library is not the mutant
    assert R.regions(g, mutant=mutant, **params) != want, (mutant, name)


def test_mutant_list_covers_the_definition():
    assert len(R.MUTANTS) >= 7 and set(R.mutant_inputs()) == set(R.MUTANTS)


def _region(w, h, x=3, y=4):
    return (0, 1, w * h, x, y, x + w - 1, y + h - 1, 0, w * h)


def test_text_box_filter_edges():
    regs = [_region(20, 30), _region(21, 30), _region(30, 10), _region(30, 11), _region(49, 12), _region(50, 12), _region(51, 12),
            _region(21, 30)]
    arr = np.array(regs, dtype=np.int32).view(_native.MSER_REGION_DTYPE).reshape(-1)
    for W in (100, 101, 102, 103):
        want = R.text_boxes(regs, W)
        assert _native.mser_text_boxes(arr, W) == want
        assert [(x, y, w, h) for x, y, w, h in want if w >= W * 0.5 or w <= 20 or h <= 10] == []
    assert [b[2] for b in _native.mser_text_boxes(arr, 100)] == [21, 30, 49, 21]                   # 50 is not below 100 * 0.5; duplicates kept
    assert [b[2] for b in _native.mser_text_boxes(arr, 101)] == [21, 30, 49, 50, 21]               # 50 < 50.5, 51 is not
    assert [b[2] for b in _native.mser_text_boxes(arr, 103)] == [21, 30, 49, 50, 51, 21]
    assert _native.mser_text_boxes(arr[:0], 100) == []
    with pytest.raises(ValueError):
        _native.mser_text_boxes(arr, 0)


def test_plan_and_refusals():
    d = _native.mser_params()
    assert (d.delta, d.min_area, d.max_area, d.max_variation, d.min_diversity) == (5, 60, 14400, 0.25, 0.2)
    for h, w in ((1, 1), (720, 1080), (4096, 4096)):
        plan = _native.mser_plan(h, w)
        assert plan["node_cap"] == h * w and h * w * 53 <= plan["workspace_bytes"] <= h * w * 53 + 12288
        assert plan["workspace_bytes"] < 1 << 30
    with pytest.raises(ValueError):
        _native.mser_plan(0, 5)
    bad = [dict(delta=0), dict(delta=256), dict(min_area=0), dict(min_area=10, max_area=9), dict(max_variation=-0.1),
           dict(max_variation=float("nan")), dict(min_diversity=-1e-9), dict(min_diversity=float("nan"))]
    for kw in bad:
        with pytest.raises(NotImplementedError):
            _native.mser_plan(8, 8, _native.mser_params(**kw))
        with pytest.raises(NotImplementedError):
            _native.mser_host(np.zeros((4, 4), np.uint8), _native.mser_params(**kw))
        with pytest.raises(NotImplementedError):
            tm.MserTextDetector(**kw)                                                              # before any device call
    for kw in (dict(delta=1), dict(delta=255), dict(min_area=7, max_area=7), dict(max_variation=0.0), dict(min_diversity=0.0)):
        _native.mser_plan(8, 8, _native.mser_params(**kw))
    with pytest.raises(NotImplementedError):
        _native.mser_plan(4097, 4096)                                                              # above the pixel cap
    with pytest.raises(ValueError):
        _native.mser_params(delta=2.5)
    for mask in (0, 4, True):
        with pytest.raises(ValueError):
            _native.mser_host(np.zeros((4, 4), np.uint8), None, mask)
    with pytest.raises(ValueError):
        _native.mser_host(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        _native.mser_tree_host(np.zeros((4, 4), np.uint8), 2)


def test_detector_refuses_before_the_device():
    det = tm.MserTextDetector()
    with pytest.raises(NotImplementedError):
        det(np.zeros((4, 4), np.float32))                                                          # dtype: the analyzer's own rule
    with pytest.raises(ValueError):
        det(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(NotImplementedError):
        det.regions_device(256, (4097, 4096))                                                      # the cap, before the pointer is used
    with pytest.raises(ValueError):
        det.regions_device(256, (4, 4, 2))


def test_analyzer_wiring_and_unchanged_default():
    img = np.zeros((8, 8, 3), np.uint8)
    ca = tm.ContentAnalyzer()
    assert ca.text_detector is None
    with pytest.raises(NotImplementedError, match="cv2.MSER is not restated"):
        ca.detect_text_regions(img)
    with pytest.raises(NotImplementedError):
        ca.create_forbidden_zone_map(img)
    with pytest.raises(NotImplementedError):
        tm.TilingModule(block_size=64, content_analyzer=ca).split_array(img)
    m = tm.ContentAnalyzer(device=0, text_detector='mser')
    assert isinstance(m.text_detector, tm.MserTextDetector) and m.text_detector.device == 0 and callable(m.text_detector)
    assert m.text_detector.params.delta == 5 and m.text_detector.params.max_area == 14400
    with pytest.raises(ValueError):
        tm.ContentAnalyzer(text_detector='ocr')
    boxes = [(1, 2, 30, 12)]
    host = tm.ContentAnalyzer(text_detector=lambda image: boxes)
    assert host.detect_text_regions(img) == boxes
    with pytest.raises(ValueError, match="host_image"):
        host._zone_rects(None, False, True, d_image=256, shape=img.shape)                          # a host callable still needs the host copy
