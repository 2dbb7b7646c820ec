"""CPU: the host side of cascade detection (csrc/sr_cascade_host.cpp, tiling_module.load_cascade) against the NumPy
restatement tests/_cascade_ref.py, the restatement against its own brute-force evaluator and against scikit-image's recorded
windows (tests/golden/cascade_skimage.npz), the scale list against hand values, the grouping on constructed lists, every
refusal by name, and the mutants of the restatement, each caught by a named input.  Everything is compared for equality."""
import functools
import math

import numpy as np
import pytest

import _cascade_ref as R
import _native
import tiling_module as tm


@functools.lru_cache(maxsize=None)
def lbp_tables():
    return tm.load_cascade(R.LBP_XML)


@functools.lru_cache(maxsize=None)
def lbp_model():
    return _native.CascadeModel(lbp_tables())


@functools.lru_cache(maxsize=None)
def fixture():
    return R.skimage_fixture()


def rows(c):
    return np.array(c, dtype=np.int64).reshape(-1, 4)


def test_loader_reads_the_fixture():
    t = lbp_tables()
    assert t["feature_type"] == "LBP" and t["window"] == (24, 24) and t["max_cat_count"] == 256 and t["max_tree_nodes"] == 1
    assert len(t["stage_thresholds"]) == 20 and t["stage_counts"].sum() == 139 and len(t["stump_feature"]) == 139
    assert t["feature_rects"].shape == (136, 4) and t["stump_subsets"].shape == (139, 8)
    assert t["stump_subsets"].dtype == np.int32 and (t["stump_subsets"] < 0).any()        # the file's signed words, 32 bits each
    assert t["stump_subsets"][0].tolist() == [-67130709, -21569, -1426120013, -1275125205, -21585, -16385, 587145899, -24005]
    assert t["stump_feature"][:3].tolist() == [46, 13, 2] and t["feature_rects"][0].tolist() == [0, 0, 3, 5]
    assert float(t["stage_thresholds"][0]) == float(np.float32(-0.7520892024040222))
    info = lbp_model().info()
    assert (info["n_stages"], info["n_stumps"], info["n_features"], info["win_w"], info["win_h"]) == (20, 139, 136, 24, 24)


def test_loader_reads_a_constructed_haar_file(tmp_path):
    """A constructed HAAR cascade written in OpenCV's new layout (float32 values printed with 9 digits) comes back as the
    same tables; a tilted rectangle, a fourth rectangle and a deeper tree are recorded for the engine to refuse."""
    t = R.random_haar(stages=(2, 3), n_feats=5)

    def xml(tilted=0, extra_rect="", extra_node=""):
        stages, k = [], 0
        for thr, cnt in zip(t["stage_thresholds"], t["stage_counts"]):
            weak = []
            for _ in range(int(cnt)):
                weak.append(f"<_><internalNodes>0 -1 {t['stump_feature'][k]} {t['stump_threshold'][k]:.9g}{extra_node}</internalNodes>"
                            f"<leafValues>{t['stump_leaves'][k][0]:.9g} {t['stump_leaves'][k][1]:.9g}</leafValues></_>")
                k += 1
            stages.append(f"<_><maxWeakCount>{cnt}</maxWeakCount><stageThreshold>{thr:.9g}</stageThreshold>"
                          f"<weakClassifiers>{''.join(weak)}</weakClassifiers></_>")
        feats = []
        for i in range(len(t["feature_nrects"])):
            rs = "".join(f"<_>{' '.join(str(int(v)) for v in t['feature_rects'][i][j])} {t['feature_weights'][i][j]:.9g}</_>"
                         for j in range(int(t["feature_nrects"][i])))
            feats.append(f"<_><rects>{rs}{extra_rect if i == 0 else ''}</rects><tilted>{tilted}</tilted></_>")
        return ('<?xml version="1.0"?><opencv_storage><cascade type_id="opencv-cascade-classifier"><stageType>BOOST</stageType>'
                f'<featureType>HAAR</featureType><height>{t["window"][1]}</height><width>{t["window"][0]}</width>'
                '<stageParams><maxWeakCount>3</maxWeakCount></stageParams><featureParams><maxCatCount>0</maxCatCount>'
                f'<featSize>1</featSize><mode>ALL</mode></featureParams><stageNum>2</stageNum><stages>{"".join(stages)}</stages>'
                f'<features>{"".join(feats)}</features></cascade></opencv_storage>')
    path = tmp_path / "haar.xml"
    path.write_text(xml())
    got = tm.load_cascade(str(path))
    assert got["feature_type"] == "HAAR" and got["window"] == t["window"] and got["tilted"] == 0 and got["max_rects"] == 3
    for key in ("stage_thresholds", "stage_counts", "stump_feature", "stump_threshold", "stump_leaves", "feature_nrects",
                "feature_rects", "feature_weights"):
        assert np.array_equal(got[key], t[key]), key
    img = R.noise_image(30, 36)
    assert np.array_equal(_native.CascadeModel(got).stage_map_host(img, 1), R.stage_map(t, img, 1))
    for kw, what in ((dict(tilted=1), "tilted"), (dict(extra_rect="<_>0 0 1 1 1.</_><_>0 0 1 1 1.</_>"), "at most 3"),
                     (dict(extra_node=" 1 2 0 0.5 -2 -3 1 0.25"), "depth-1")):
        path.write_text(xml(**kw))
        with pytest.raises(NotImplementedError, match=what):
            _native.CascadeModel(tm.load_cascade(str(path)))


def test_restatement_equals_brute_force():
    f = fixture()
    plane = f["plane72"][10:44, 12:48]                                                    # around the face: windows go deep
    assert np.array_equal(R.stage_map(lbp_tables(), plane, 1), R.stage_map(lbp_tables(), plane, 1, brute=True))
    hm, img, _ = R.HAAR_INPUTS["wide_window"]()
    img = img[:, :45]
    a, b = R.stage_map(hm, img, 1), R.stage_map(hm, img, 1, brute=True)
    assert np.array_equal(a, b) and a.max() > 1
    assert R.candidates(R.noise_image(30, 40), R.random_lbp()) == R.candidates(R.noise_image(30, 40), R.random_lbp(), brute=True)


@pytest.mark.parametrize("side", [72, 80, 88])
def test_scale_one_windows_equal_scikit_image(side):
    """PINNED PARITY: the windows that pass all 20 stages of the OpenCV-trained model equal skimage.feature.Cascade's."""
    f = fixture()
    plane, want = f[f"plane{side}"], f[f"windows{side}"]
    assert len(want) >= 1
    ref = R.stage_map(lbp_tables(), plane, 1)
    assert np.argwhere(ref == 20).tolist() == want.tolist()
    for step in (1, 2):
        host = lbp_model().stage_map_host(plane, step)
        assert np.array_equal(host, ref[::step, ::step])
    assert np.argwhere(lbp_model().stage_map_host(plane, 1) == 20).tolist() == want.tolist()


def test_host_twin_equals_restatement():
    for model, img, kw in ((R.random_lbp(), R.noise_image(56, 64), {}), (R.random_lbp(), R.noise_image(41, 90, 4), dict(scale_factor=1.3)),
                           (R.checker(), R.checker_image(40, 52), {}), (R.accept_all(), R.noise_image(30, 27), {}),
                           (R.reject_all(), R.noise_image(30, 27), {})):
        m = _native.CascadeModel(model)
        want = R.candidates(img, model, **kw)
        got = m.host(img, _native.cascade_params(**kw))
        assert np.array_equal(rows(got), rows(want))
        assert np.array_equal(m.stage_map_host(img, 2), R.stage_map(model, img, 2))
        for k, p in enumerate(R.planes(img, model, **kw)):
            assert np.array_equal(m.plane_host(img, k, _native.cascade_params(**kw)), p)
    assert len(R.candidates(R.noise_image(56, 64), R.random_lbp())) > 0


def test_crop_boxes_meet_scikit_images_box():
    """The whole pipeline on the 256 x 256 crop with the defaults: the host twin equals the restatement, and a grouped box
    and scikit-image's own multi-scale box contain each other's centre (a condition on the definition)."""
    f = fixture()
    want = R.candidates(f["crop"], lbp_tables())
    got = lbp_model().host(f["crop"])
    assert np.array_equal(rows(got), rows(want)) and len(want) >= 5
    boxes = R.group(want, 4)
    assert np.array_equal(rows(_native.cascade_group(got, 4)), rows(boxes)) and len(boxes) >= 1
    r, c, w, h = (int(v) for v in f["multiscale_box"])
    ok = [b for b in boxes if b[0] <= c + w / 2 <= b[0] + b[2] and b[1] <= r + h / 2 <= b[1] + b[3]
          and c <= b[0] + b[2] / 2 <= c + w and r <= b[1] + b[3] / 2 <= r + h]
    assert ok, (boxes, (c, r, w, h))


def scales_of(model, h, w, **kw):
    return [(s["sw"], s["sh"], s["win_w"], s["win_h"], s["step"], s["nx"], s["ny"])
            for s in _native.CascadeModel(model).plan(h, w, _native.cascade_params(**kw))["scales"]]


def test_scale_list_against_hand_values():
    a = R.accept_all()
    # 100 x 60, factor 1.2: f = 1, 1.2, 1.44, 1.728, 2.0736, 2.48832; the next window (72) is above the image
    assert scales_of(a, 60, 100, scale_factor=1.2) == [(100, 60, 24, 24, 2, 39, 19), (83, 50, 29, 29, 2, 30, 14), (69, 42, 35, 35, 2, 23, 10),
                                                        (58, 35, 41, 41, 2, 18, 6), (48, 29, 50, 50, 1, 25, 6), (40, 24, 60, 60, 1, 17, 1)]
    assert scales_of(a, 60, 100, scale_factor=2.5) == [(100, 60, 24, 24, 2, 39, 19), (40, 24, 60, 60, 1, 17, 1)]
    # 60 x 30, factor 1.1: 30 / 1.331 = 22.5 rows are fewer than the window
    assert scales_of(a, 30, 60, scale_factor=1.1) == [(60, 30, 24, 24, 2, 19, 4), (55, 27, 26, 26, 2, 16, 2), (50, 25, 29, 29, 2, 14, 1)]
    # half to even: 5 * 2.5 = 12.5 -> 12
    assert [s[2] for s in scales_of(R.accept_all((5, 5)), 50, 50, scale_factor=2.5)] == [5, 12, 31]
    for h, w, kw in ((60, 100, dict(scale_factor=1.2)), (256, 256, {}), (50, 77, dict(scale_factor=1.1, min_size=(30, 30), max_size=(45, 40)))):
        got = scales_of(a, h, w, **kw)
        assert got == [(s["sw"], s["sh"], s["win_w"], s["win_h"], s["step"], s["nx"], s["ny"]) for s in R.scale_list(w, h, a, **kw)]
    assert [s[2] for s in scales_of(a, 50, 77, scale_factor=1.1, min_size=(30, 30), max_size=(45, 40))] == [32, 35, 39]
    assert scales_of(a, 23, 100) == [] and scales_of(a, 100, 23) == []
    plan = _native.CascadeModel(a).plan(60, 100, _native.cascade_params(scale_factor=2.5))
    assert plan["positions"] == 39 * 19 + 17 and plan["workspace_bytes"] > 6000 + 960 + 4 * (101 * 61 + 41 * 25)


def test_step_switches_at_two():
    a = R.accept_all()
    assert [s[4] for s in scales_of(a, 100, 100, scale_factor=2.0)] == [2, 2, 1]           # f = 1, 2, 4
    assert [s[4] for s in scales_of(a, 100, 100, scale_factor=math.nextafter(2.0, 3.0))] == [2, 1, 1]


def test_resize():
    m = _native.CascadeModel(R.accept_all((3, 3)))
    p15 = _native.cascade_params(scale_factor=1.5)
    img = R.noise_image(6, 6)
    assert np.array_equal(m.plane_host(img, 0, p15), img)                                 # f = 1 is the identity
    assert np.array_equal(m.plane_host(np.full((6, 6), 173, np.uint8), 1, p15), np.full((4, 4), 173, np.uint8))
    # 6 -> 4 samples sit at 0.25, 1.75, 3.25, 4.75: on the ramp 0, 10, .. 50 that is 2.5, 17.5, 32.5, 47.5, halves rounded up
    ramp = np.tile(np.arange(0, 60, 10, dtype=np.uint8), (6, 1))
    assert m.plane_host(ramp, 1, p15).tolist() == [[3, 18, 33, 48]] * 4
    assert m.plane_host(ramp.T.copy(), 1, p15).tolist() == [[v] * 4 for v in (3, 18, 33, 48)]
    # 7 -> 3 samples sit at 2 / 3, 3, 16 / 3: thirds, weights 2 and 4 over the denominator 6
    wide = np.tile(np.array([0, 30, 60, 90, 120, 150, 180], np.uint8), (7, 1))
    assert R.resize(wide, 3, 3).tolist() == [[20, 90, 160]] * 3
    assert np.array_equal(_native.CascadeModel(R.accept_all((3, 3))).plane_host(wide, 1, _native.cascade_params(scale_factor=2.2)),
                          R.resize(wide, 3, 3))
    assert np.array_equal(R.resize(ramp, 6, 6), ramp)


def test_grouping_on_constructed_lists():
    def both(cands, mn):
        got = rows(_native.cascade_group(cands, mn)).tolist()
        assert got == rows(R.group(cands, mn)).tolist()
        return [tuple(r) for r in got]
    chain = [(0, 0, 20, 20), (3, 0, 20, 20), (6, 0, 20, 20)]                               # delta 4: 0-3 and 3-6 similar, 0-6 not
    assert both(chain, 2) == [(3, 0, 20, 20)] and both(chain[::2], 1) == [] and both(chain[:2], 1) == [(2, 0, 20, 20)]
    one = (10, 12, 30, 30)
    assert both([one] * 4, 4) == [] and both([one] * 5, 4) == [one]
    small, big = (40, 40, 20, 20), (20, 20, 60, 60)                                        # small lies inside big; they are not similar
    assert both([small] * 3 + [big] * 4, 1) == [big]                                       # n2 = 4 > max(3, 3)
    assert both([small] * 3 + [big] * 3, 1) == [small, big]                                # n2 = 3 is not
    assert both([small] * 4 + [big] * 5, 1) == [big] and both([small] * 4 + [big] * 4, 1) == [small, big]
    assert both([small] * 2 + [big] * 2, 1) == [big]                                       # n1 < 3
    assert both([big] * 2 + [small] * 2, 1) == [big]                                       # classes keep the order of their first member
    assert both([small] * 3 + [big] * 1, 1) == [small]                                     # a class below min_neighbors contains nothing
    assert both([small, big, small], 0) == [small, big, small] and both([], 3) == []
    # a long class far from the origin: 1100 members with x near 2 000 000 sum to 2.2e9, beyond an int: the sums are held in
    # 64 bits (their float32 image times the float32 1 / 1100 rounds to 2000001)
    far = [(2000000 + i % 3, 5, 40, 40) for i in range(1100)]
    assert both(far, 3) == [(2000001, 5, 40, 40)]
    # the mean: int sums times the float32 1 / n, half to even: (1 + 2) / 2 = 1.5 -> 2, (2 + 3) / 2 = 2.5 -> 2
    assert both([(1, 2, 20, 20), (2, 3, 20, 20)], 1) == [(2, 2, 20, 20)]


def _haar_tables(**over):
    t = dict(R.random_haar())
    t.update(over)
    return t


def _lbp_tables(**over):
    t = dict(R.random_lbp())
    t.update(over)
    return t


def test_every_refusal_by_name(tmp_path):
    def refused(what, fn):
        with pytest.raises(NotImplementedError, match=what):
            fn()
    old = tmp_path / "old.xml"
    old.write_text('<?xml version="1.0"?><opencv_storage><haarcascade_frontalface_default type_id="opencv-haar-classifier">'
                   '<size>24 24</size><stages></stages></haarcascade_frontalface_default></opencv_storage>')
    refused("old opencv-haar-classifier", lambda: _native.CascadeModel(tm.load_cascade(str(old))))
    refused("old opencv-haar-classifier", lambda: tm.CascadeFaceDetector(str(old)))
    M = _native.CascadeModel
    refused("BOOST", lambda: M(_lbp_tables(stage_type=1)))
    refused("depth-1", lambda: M(_lbp_tables(max_tree_nodes=3)))
    refused("tilted", lambda: M(_haar_tables(tilted=1)))
    refused("at most 3", lambda: M(_haar_tables(max_rects=4)))
    nr = R.random_haar()["feature_nrects"].copy()
    nr[R.random_haar()["stump_feature"][0]] = 1
    refused("2 or 3", lambda: M(_haar_tables(feature_nrects=nr)))
    refused("maxCatCount", lambda: M(_lbp_tables(max_cat_count=128)))
    refused("HOG", lambda: M(_lbp_tables(feature_type="HOG")))
    for win in ((2, 24), (24, 256), (256, 256)):
        refused("window", lambda: M(R.accept_all(win)))
    refused("zero stages", lambda: M(dict(R.accept_all(), stage_thresholds=np.zeros(0, np.float32), stage_counts=np.zeros(0, np.int32))))
    sf = R.random_lbp()["stump_feature"].copy()
    sf[5] = 12
    refused("names feature", lambda: M(_lbp_tables(stump_feature=sf)))
    fr = R.random_lbp()["feature_rects"].copy()
    fr[:, 0] = 24 - 3 * fr[:, 2] + 1
    refused("outside the window", lambda: M(_lbp_tables(feature_rects=fr)))
    hr = R.random_haar()["feature_rects"].copy()
    hr[:, 0, 3] = 17
    refused("outside the window", lambda: M(_haar_tables(feature_rects=hr)))
    nan = np.float32("nan")
    for key, shape in (("stage_thresholds", None), ("stump_leaves", None), ("stump_threshold", None), ("feature_weights", None)):
        bad = R.random_haar()[key].copy()
        bad.reshape(-1)[0] = nan
        refused("NaN", lambda: M(_haar_tables(**{key: bad})))
    m = lbp_model()
    for sfac in (1.0, 0.9, float("nan")):
        refused("scale_factor", lambda: m.plan(100, 100, _native.cascade_params(scale_factor=sfac)))
        refused("scale_factor", lambda: tm.CascadeFaceDetector(lbp_tables(), scale_factor=sfac))
    refused("steps in the scale list", lambda: m.plan(4096, 4096, _native.cascade_params(scale_factor=1.01)))
    assert len(m.plan(4096, 4096, _native.cascade_params(scale_factor=1.05))["scales"]) == 106
    refused("min_neighbors", lambda: m.plan(100, 100, _native.cascade_params(min_neighbors=-1)))
    refused("min_neighbors", lambda: _native.cascade_group([(0, 0, 5, 5)], -1))
    refused("above the cap", lambda: m.plan(4097, 4096))
    # neither the pixel cap nor the step cap bounds the pyramid at a factor close to 1: 125 scales of 24 x 699050 hold
    # 2 162 340 575 table elements, 119 scales of 3 x 5592405 hold 2 468 023 484 -- more than an int32 index reaches
    thin = _native.cascade_params(scale_factor=1.000165, max_size=(24, 24))
    refused("table elements", lambda: M(R.accept_all()).plan(24, 699050, thin))
    refused("table elements", lambda: M(R.accept_all((3, 3))).plan(3, 5592405, _native.cascade_params(scale_factor=1.0013)))
    refused("table elements", lambda: tm.CascadeFaceDetector(R.accept_all((3, 3)), scale_factor=1.0013).candidates_device(1, (3, 5592405)))
    below = M(R.accept_all()).plan(24, 699050, _native.cascade_params(scale_factor=1.0002, max_size=(24, 24)))      # 1 798 942 375
    assert len(below["scales"]) == 104 and sum((s["sw"] + 1) * (s["sh"] + 1) for s in below["scales"]) < 2 ** 31
    assert m.plan(4096, 4096)["workspace_bytes"] < 1 << 30
    with pytest.raises(NotImplementedError, match="above the cap"):
        m.host(np.zeros((1, 2 ** 24 + 1), np.uint8))
    with pytest.raises(ValueError):
        m.plan(0, 10)
    with pytest.raises(ValueError):
        M(_lbp_tables(stump_leaves=np.zeros((3, 2), np.float32)))


def test_default_analyzer_is_unchanged(caplog):
    ca = tm.ContentAnalyzer()
    assert ca.face_detector is None and ca.face_cascade is None
    with caplog.at_level("INFO", logger="tiling_module"):
        assert ca.detect_faces(np.zeros((8, 8, 3), np.uint8)) == []
    assert "no face detector given; detect_faces returns []" in caplog.text
    ca = tm.ContentAnalyzer(face_cascade=R.LBP_XML)
    assert isinstance(ca.face_detector, tm.CascadeFaceDetector) and ca.face_cascade is ca.face_detector.model
    assert ca.face_detector.params.scale_factor == 1.1 and ca.face_detector.params.min_neighbors == 4
    with pytest.raises(ValueError):
        tm.ContentAnalyzer(face_cascade=R.LBP_XML, face_detector=lambda img: [])


# ---- Haar: constructed cascades only -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.HAAR_INPUTS))
def test_haar_host_equals_restatement_with_a_margin(name):
    """Equality must not rest on the last bit of a square root: on every stump evaluated |val - thr nf| stays above
    1e-9 max(|val|, |thr nf|) in the restatement; an input that does not is a failed test."""
    model, img, kw = R.HAAR_INPUTS[name]()
    margins = R.Margins()
    want = R.candidates(img, model, margins=margins, **kw)
    smap = R.stage_map(model, img, 1, margins=margins)
    print(f"{name}: {img.shape}, worst margin {margins.worst:.3e}, {len(want)} candidates, deepest window {smap.max()}")
    assert margins.worst > 1e-9
    m = _native.CascadeModel(model)
    assert np.array_equal(rows(m.host(img, _native.cascade_params(**kw))), rows(want))
    assert np.array_equal(m.stage_map_host(img, 1), smap)
    assert smap.max() >= 2 and (name != "flat" or (smap[2:6, 3:9] == smap[2, 3]).all())


# ---- mutants of the restatement, each caught by a named input ----------------------------------------------------------------
def test_mutants_are_caught():
    f = fixture()
    real, plane = lbp_tables(), f["plane80"][12:56, 16:60]
    base = R.stage_map(real, plane, 1)
    assert np.array_equal(lbp_model().stage_map_host(plane, 1), base) and (base == 20).sum() == 2
    for mut in ("bit_order", "subset_inverted"):                                           # named input: the face of the 80-pixel plane
        assert not np.array_equal(R.stage_map(real, plane, 1, mut=mut), base), mut
    flat = np.full((24, 24), 90, np.uint8)                                                 # named input: a flat window, every block ties
    assert R.stage_map(real, flat, 1).tolist() == lbp_model().stage_map_host(flat, 1).tolist() != R.stage_map(real, flat, 1, mut="strict").tolist()
    edge = R._lbp((24, 24), [(0.0, [])], [])                                               # named input: a stage whose sum equals its threshold
    img = R.noise_image(24, 24)
    assert R.stage_map(edge, img, 1).tolist() == [[1]] == _native.CascadeModel(edge).stage_map_host(img, 1).tolist()
    assert R.stage_map(edge, img, 1, mut="stage_le").tolist() == [[0]]
    a, host_a = R.accept_all(), _native.CascadeModel(R.accept_all())
    img26 = R.noise_image(26, 26)                                                          # named input: 26 x 26, 2 x 2 positions (and one at f = 1.1)
    assert len(R.candidates(img26, a)) == 5 == len(host_a.host(img26)) and len(R.candidates(img26, a, mut="step1")) == 10
    assert len(R.candidates(img, a)) == 1 == len(host_a.host(img)) and R.candidates(img, a, mut="exclusive_last") == []   # exactly 24 x 24
    img96 = R.noise_image(80, 96)                                                          # named input: 96 x 80, x = 6 at f = 1.1 is 6.6
    want = R.candidates(img96, a)
    assert np.array_equal(rows(host_a.host(img96)), rows(want)) and (7, 0, 26, 26) in want
    assert R.candidates(img96, a, mut="floor_candidate") != want
    model, himg, kw = R.HAAR_INPUTS["noise"]()                                             # named input: the Haar noise case
    assert not np.array_equal(R.stage_map(model, himg, 1, mut="norm_whole"), R.stage_map(model, himg, 1))
    five = [(10, 12, 30, 30)] * 4                                                          # named input: a class of exactly min_neighbors
    assert R.group(five, 4) == [] == rows(_native.cascade_group(five, 4)).tolist() and R.group(five, 4, mut="n_lt") == [(10, 12, 30, 30)]
