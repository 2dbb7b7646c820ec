"""CPU: the NumPy restatement of ContentAnalyzer (tests/_content_ref.py) against independent forms on small arrays, the
fixtures of the GPU tests (non-degenerate spectrum, a salient spot), and the mirror's argument checks, every one of which
raises before any device work (there is no device here)."""
import numpy as np
import pytest

import _content_ref as R
import tiling_module as tm


def _dft2_direct(a):
    h, w = a.shape
    wy = np.exp(-2j * np.pi * np.outer(np.arange(h), np.arange(h)) / h)
    wx = np.exp(-2j * np.pi * np.outer(np.arange(w), np.arange(w)) / w)
    return wy @ a.astype(np.complex128) @ wx


def _refl101(p, n):
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def _saliency_loops(img):
    """The saliency with a direct O(N^2) DFT, an explicitly shifted array and loop-form filters."""
    g = R.gray_bgr_rule(img).astype(np.float64)
    h, w = g.shape
    F = _dft2_direct(g)
    sh = np.empty_like(F)
    for u in range(h):
        for k in range(w):
            sh[(u + h // 2) % h, (k + w // 2) % w] = F[u, k]
    L = np.log(np.abs(sh) + 1e-8)
    avg = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            avg[y, x] = sum(L[_refl101(y + i, h), _refl101(x + j, w)] / 25.0 for i in range(-2, 3) for j in range(-2, 3))
    G = np.exp(L - avg) * np.where(np.abs(sh) == 0, 1.0, sh / np.where(np.abs(sh) == 0, 1.0, np.abs(sh)))
    un = np.empty_like(G)
    for u in range(h):
        for k in range(w):
            un[u, k] = G[(u + h // 2) % h, (k + w // 2) % w]
    s = np.abs(np.conj(_dft2_direct(np.conj(un))) / (h * w))
    k5 = np.array([1, 4, 6, 4, 1]) / 16.0
    out = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            out[y, x] = sum(k5[i + 2] * k5[j + 2] * s[_refl101(y + i, h), _refl101(x + j, w)]
                            for i in range(-2, 3) for j in range(-2, 3))
    return out


@pytest.mark.parametrize("h,w,cn", [(16, 16, 3), (9, 14, 3), (7, 5, 1), (1, 12, 3), (11, 1, 4), (3, 2, 3)])
def test_saliency_restatement_matches_loop_form(h, w, cn):
    img = R.synthetic(h, w, cn, seed=3)
    want = _saliency_loops(img)
    got = R.saliency_float(img)
    assert np.allclose(got, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
    assert R.saliency(img).dtype == np.uint8 and R.saliency(img).shape == (h, w)


def test_pad101_is_cv2_iterated_reflection():
    for n in (1, 2, 3, 4, 7):
        a = np.arange(n, dtype=np.float64)[None, :]
        P = R.pad101(a, 2)
        assert P.shape == (5, n + 4)
        assert [P[2, 2 + x] for x in range(-2, n + 2)] == [float(_refl101(x, n)) for x in range(-2, n + 2)]


def test_gray_rule_swaps_red_and_blue():
    img = np.zeros((1, 3, 3), np.uint8)
    img[0, 0, 0] = img[0, 1, 1] = img[0, 2, 2] = 255
    assert R.gray_bgr_rule(img).tolist() == [[29, 150, 76]]           # channel 0 weighs as blue
    g = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(R.gray_bgr_rule(g), g) and np.array_equal(R.gray_bgr_rule(g[..., None]), g)


@pytest.mark.parametrize("win", [1, 3, 7, 64])
def test_entropy_restatement_matches_unique_counts(win):
    img = R.synthetic(23, 31, 3, seed=5)
    g = R.gray_bgr_rule(img)
    got = R.local_entropy(img, win)
    assert got.dtype == np.float32
    for y in range(0, 23, win):
        for x in range(0, 31, win):
            cell = g[y:y + win, x:x + win]
            _, c = np.unique(cell, return_counts=True)
            p = c / c.sum()
            want = -np.sum(p * np.log2(p))
            assert np.all(got[y:y + win, x:x + win] == got[y, x])
            assert abs(float(got[y, x]) - want) < 2e-5


def test_forbidden_map_and_flags_match_python_loops():
    img = R.synthetic(40, 60, 3)
    sal = R.saliency(img)
    faces, texts = [(50, 30, 20, 10), (2, 3, 5, 9)], [(55, 35, 30, 30), (0, 0, 4, 2)]
    fm = R.forbidden_map(img, faces, texts, True, 0.7)
    want = np.zeros((40, 60), bool)
    for y in range(40):
        for x in range(60):
            v = sal[y, x] > 178
            for (bx, by, bw, bh) in faces:
                m = int(max(bw, bh) * 0.2)
                v = v or (max(0, bx - m) <= x < bx + bw + m and max(0, by - m) <= y < by + bh + m)
            for (bx, by, bw, bh) in texts:
                v = v or (bx <= x < bx + bw and by <= y < by + bh)
            want[y, x] = v
    assert np.array_equal(fm, want)
    positions = [(0, 0, 32, 32), (28, 0, 32, 32), (0, 8, 32, 32), (28, 8, 32, 32), (50, 30, 32, 32)]
    flags = R.tile_flags(fm, positions)
    for (x, y, w, h), f in zip(positions, flags):
        cnt = tot = 0
        for yy in range(y, min(y + h, 40)):
            for xx in range(x, min(x + w, 60)):
                tot += 1
                cnt += bool(want[yy, xx])
        assert f == {'has_forbidden_zone': cnt > 0, 'forbidden_ratio': cnt / tot}


@pytest.mark.parametrize("h,w,cn", R.SALIENCY_CASES)
def test_gpu_fixtures_are_not_degenerate(h, w, cn):
    img = R.synthetic(h, w, cn)
    assert img.shape[:2] == (h, w) and img.dtype == np.uint8
    assert R.min_spectrum_magnitude(img) > 1.0
    assert int((R.saliency(img) > int(255 * 0.7)).sum()) >= 1


# ---- the mirror's argument checks: each raises before device work -------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(tm._native, "default_context", boom)


def test_wrong_dtype_raises_not_implemented(no_device):
    ca = tm.ContentAnalyzer()
    for dt in (np.float32, np.float64, np.uint16, np.int8):
        img = np.zeros((8, 8, 3), dt)
        with pytest.raises(NotImplementedError):
            ca.compute_saliency_map(img)
        with pytest.raises(NotImplementedError):
            ca.compute_local_entropy(img)
        with pytest.raises(NotImplementedError):
            ca.create_forbidden_zone_map(img, protect_text=False)


def test_bad_shape_raises_value_error(no_device):
    ca = tm.ContentAnalyzer()
    for shape in ((8,), (8, 8, 2), (8, 8, 5), (2, 8, 8, 3), (0, 8), (8, 0, 3)):
        img = np.zeros(shape, np.uint8)
        with pytest.raises(ValueError):
            ca.compute_saliency_map(img)
        with pytest.raises(ValueError):
            ca.compute_local_entropy(img)
        with pytest.raises(ValueError):
            ca.create_forbidden_zone_map(img, protect_text=False)
    with pytest.raises(ValueError):
        ca.compute_saliency_map_device(0, (8, 8, 2))
    with pytest.raises(ValueError):
        ca.compute_local_entropy(np.zeros((8, 8), np.uint8), window_size=0)


def test_text_protection_without_detector_raises_before_device_work(no_device):
    ca = tm.ContentAnalyzer()
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(NotImplementedError):
        ca.detect_text_regions(img)
    with pytest.raises(NotImplementedError):
        ca.create_forbidden_zone_map(img)                       # protect_text defaults to True
    with pytest.raises(NotImplementedError):
        ca.create_forbidden_zone_map_device(0, (8, 8, 3))
    assert ca.detect_faces(img) == []


def test_side_above_fft_limit_raises_not_implemented(no_device, monkeypatch):
    monkeypatch.setattr(tm, "_FFT_MAX_LEN", 16)
    ca = tm.ContentAnalyzer()
    for shape in ((17, 4, 3), (4, 17)):
        img = np.zeros(shape, np.uint8)
        with pytest.raises(NotImplementedError):
            ca.compute_saliency_map(img)
        with pytest.raises(NotImplementedError):
            ca.create_forbidden_zone_map(img, protect_text=False)
        with pytest.raises(NotImplementedError):
            ca.create_forbidden_zone_map_device(0, shape, protect_text=False)


def test_fft_limit_constant_matches_the_library():
    assert tm._FFT_MAX_LEN == tm._native.load().sr_fft_max_len()


def test_detectors_are_host_callables():
    ca = tm.ContentAnalyzer(face_detector=lambda im: [(np.int32(1), 2, 3, 4)], text_detector=lambda im: [(5, 6, 7, 8)])
    img = np.zeros((8, 8, 3), np.uint8)
    assert ca.detect_faces(img) == [(1, 2, 3, 4)] and ca.detect_text_regions(img) == [(5, 6, 7, 8)]
    assert ca._zone_rects(img, True, True) == [(1, 2, 3, 4), (5, 6, 7, 8)]        # margin int(4 * 0.2) = 0
    big = tm.ContentAnalyzer(face_detector=lambda im: [(3, 20, 10, 30)])
    assert big._zone_rects(img, True, False) == [(0, 14, 19, 42)]                 # margin 6, clipped at x = 0


def test_tiling_module_default_has_no_analyzer(tmp_path, no_device):
    t = tm.TilingModule(block_size=64, l2_cache_dir=str(tmp_path))
    assert t.content_analyzer is None and t.enable_content_aware is True
    ca = tm.ContentAnalyzer()
    t2 = tm.TilingModule(block_size=64, l2_cache_dir=str(tmp_path), content_analyzer=ca,
                         forbidden_zone_args={'protect_text': False})
    assert t2.content_analyzer is ca and t2.forbidden_zone_args == {'protect_text': False}
    with pytest.raises(ValueError):
        tm.TilingModule(block_size=64, l2_cache_dir=str(tmp_path), device=1, content_analyzer=ca)
    # protect_text (default True) without a text detector: refused before the image is uploaded
    t3 = tm.TilingModule(block_size=64, l2_cache_dir=str(tmp_path), content_analyzer=ca)
    with pytest.raises(NotImplementedError):
        t3.split_array(np.zeros((80, 80, 3), np.uint8))
