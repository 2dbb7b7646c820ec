"""CPU: the NumPy restatement of the commercial / no-reference metrics (tests/_commercial_ref.py) against independent
forms, and the host side of QualityAssessmentModule.evaluate_commercial / evaluate_no_reference: argument validation
before any device call, key order, levels, the composite score and JSON-clean values -- with the device sums replaced
by the restatement's."""
import json

import numpy as np
import pytest

import _commercial_ref as R
import _native
import quality_assessment_module as qam


# ---- the restatement against independent forms ------------------------------------------------------------------------

def test_canny_components_equal_literal_stack_port():
    rng = np.random.default_rng(3)
    imgs = [(rng.integers(0, 4, (40, 53)) * 25).astype(np.uint8), rng.integers(0, 256, (37, 29), dtype=np.uint8),
            np.tile(np.arange(30, dtype=np.uint8) * 7, (20, 1)), np.zeros((1, 9), np.uint8), np.full((5, 1), 200, np.uint8)]
    yy, xx = np.mgrid[0:64, 0:64]
    imgs.append(np.where((yy - 32) ** 2 + (xx - 30) ** 2 < 300, 140, 100).astype(np.uint8))
    for img in imgs:
        g = R.gray_of(img)
        assert np.array_equal(R.canny_edges(g), R.canny_edges_stack(g))


def test_hf_ratio_fp32_against_fp64():
    rng = np.random.default_rng(4)
    for h, w in ((64, 80), (97, 61), (1, 17), (33, 1), (128, 128)):
        g = R.gray_of(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        f32 = R.hf_ratio(g, fft2=lambda a: np.fft.fft2(a.astype(np.float32)).astype(np.complex64))
        assert f32 == pytest.approx(R.hf_ratio(g), rel=1e-4, abs=1e-7)


def test_lab_tables_against_float_cie():
    rng = np.random.default_rng(5)
    c = rng.integers(0, 256, (20000, 3)).astype(np.uint8)
    c[:8] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [128, 128, 128], [1, 2, 3], [250, 5, 128]]
    lab = R.rgb2lab8(c[None])[0].astype(np.float64)
    x = c / 255.0
    lin = np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
    m = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    xyz = lin @ m.T / np.array([0.950456, 1.0, 1.088754])
    f = np.where(xyz > 216 / 24389, np.cbrt(xyz), xyz * 841 / 108 + 16 / 116)
    ref = np.stack([(116 * f[:, 1] - 16) * 255 / 100, 500 * (f[:, 0] - f[:, 1]) + 128, 200 * (f[:, 1] - f[:, 2]) + 128], -1)
    d = np.abs(lab - np.clip(np.rint(ref), 0, 255))
    # the fixed-point path (tables, 12-bit coefficients) stays within one code of the rounded float formula for L and b
    # and within two for a (500 x the cube-root step)
    assert d[:, 0].max() <= 1 and d[:, 2].max() <= 1 and d[:, 1].max() <= 2
    assert (d <= 1).mean() > 0.99
    assert lab[1].tolist() == [255, 128, 128] and lab[2].tolist() == [136, 208, 195]
    # the module's host rule (brand delta E) is the same table rule
    for col in c[:200]:
        assert np.array_equal(qam._lab8(col), R.rgb2lab8(col[None, None])[0, 0])


@pytest.mark.parametrize("h", [3, 8, 9, 16, 17])
@pytest.mark.parametrize("w", [3, 8, 9, 16])
def test_block_and_region_quirks(h, w):
    rng = np.random.default_rng(h * 100 + w)
    g = rng.integers(0, 256, (h, w)).astype(np.int64)
    ny, nx = len(range(0, h - 8, 8)), len(range(0, w - 8, 8))
    assert ny == (max(h - 8, 0) + 7) // 8 and nx == (max(w - 8, 0) + 7) // 8   # the kernel's count (sr_commercial_u8)
    row = np.zeros(40, np.int64)
    b = g[:ny * 8, :nx * 8].reshape(ny, 8, nx, 8)
    v = (64 * (b * b).sum((1, 3)) - b.sum((1, 3)) ** 2).ravel()
    row[17], q, row[38] = v.sum(), int((v * v).sum()), ny * nx
    row[18], row[19] = q & 0xffffffff, q >> 32
    assert qam.QualityAssessmentModule._artifact_of(row) == pytest.approx(R.artifact_score(g), rel=1e-12)
    rh, rw = h // 4, w // 4
    for k in range(16):
        row[20 + k] = g[(k // 4) * rh:(k // 4 + 1) * rh, (k % 4) * rw:(k % 4 + 1) * rw].sum()
    with np.errstate(invalid="ignore"), pytest.warns(RuntimeWarning) if (rh == 0 or rw == 0) else _nullctx():
        ref = R.brightness_uniformity(g) if rh and rw else _reference_uniformity(g)
    assert qam.QualityAssessmentModule._uniformity_of(row, h, w) == ref
    if h <= 8 or w <= 8:
        assert R.artifact_score(g) == 100.0


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _reference_uniformity(g):
    """The reference's literal loop: empty regions give NaN means and max(0, nan) is 0."""
    h, w = g.shape
    rh, rw = h // 4, w // 4
    means = [np.mean(g[i * rh:(i + 1) * rh, j * rw:(j + 1) * rw]) for i in range(4) for j in range(4)]
    return float(max(0, 100 - np.std(means)))


# ---- host surface -----------------------------------------------------------------------------------------------------

def _sums(img, flags, rois=(), roi_flags=()):
    """What sr_commercial_u8 returns, computed by the restatement (include/sr_hip.h slot layout)."""
    g = R.gray_of(img)
    H, W = g.shape
    rects = [((0, 0, W, H), flags)] + list(zip(rois, roi_flags))
    ints = np.zeros((len(rects), 40), np.int64)
    flts = np.zeros((len(rects), 8), np.float64)
    for k, ((x, y, w, h), f) in enumerate(rects):
        sub, gs = img[y:y + h, x:x + w], g[y:y + h, x:x + w]
        r, fl = ints[k], flts[k]
        lap = R.laplacian(gs)
        r[0:4] = lap.sum(), (lap * lap).sum(), gs.sum(), (gs * gs).sum()
        n16 = R.noise16(gs)
        r[4:6] = n16.sum(), (n16 * n16).sum()
        gx, gy = R.sobel(gs)
        r[6] = (gx * gx + gy * gy).sum()
        fl[3] = np.sqrt((gx * gx + gy * gy).astype(np.float64)).sum()
        m = R.mscn(gs).astype(np.float64)
        fl[0:3] = m.sum(), (m * m).sum(), np.abs(m).sum()
        fl[4] = R.local_variance5(gs).astype(np.float64).sum()
        if img.ndim == 3:
            lab = R.rgb2lab8(sub).astype(np.int64).reshape(-1, 3)
            r[7:13] = lab[:, 0].sum(), (lab[:, 0] ** 2).sum(), lab[:, 1].sum(), (lab[:, 1] ** 2).sum(), lab[:, 2].sum(), \
                (lab[:, 2] ** 2).sum()
            ycc = R.rgb2ycrcb8(sub)
            r[13] = ((ycc[..., 1] >= 133) & (ycc[..., 1] <= 173) & (ycc[..., 2] >= 77) & (ycc[..., 2] <= 127)).sum()
            r[14:17] = sub[..., :3].reshape(-1, 3).astype(np.int64).sum(0)
    r, fl = ints[0], flts[0]
    ny, nx = len(range(0, H - 8, 8)), len(range(0, W - 8, 8))
    b = g[:ny * 8, :nx * 8].reshape(ny, 8, nx, 8)
    v = (64 * (b * b).sum((1, 3)) - b.sum((1, 3)) ** 2).ravel()
    q = int((v * v).sum())
    r[17], r[18], r[19], r[38] = v.sum(), q & 0xffffffff, q >> 32, ny * nx
    rh, rw = H // 4, W // 4
    for k in range(16):
        r[20 + k] = g[(k // 4) * rh:(k // 4 + 1) * rh, (k % 4) * rw:(k % 4 + 1) * rw].sum()
    r[36] = R.canny_edges(g).sum()
    F = np.abs(np.fft.fftshift(np.fft.fft2(g.astype(np.float64))))
    yy, xx = np.ogrid[:H, :W]
    fl[6], fl[5] = F.sum(), F[(xx - W // 2) ** 2 + (yy - H // 2) ** 2 > (min(H, W) // 4) ** 2].sum()
    return ints, flts


class _FakeQA(qam.QualityAssessmentModule):
    """The module with the device replaced by the restatement's sums."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.calls = 0

    def _ctx(self):
        return None

    def evaluate_commercial(self, image, roi_regions=None):
        img = self._commercial_image(image, "evaluate_commercial")
        plan = self._roi_plan(img.shape, roi_regions)
        d = qam._DevImage.__new__(qam._DevImage)
        d.ctx, d.buf, d._ptr, d.shape, d.img = None, None, 0, img.shape, img
        return self._evaluate_commercial_dev(d, plan)

    def _cm_sums(self, d, flags, rois=(), roi_flags=()):
        self.calls += 1
        return _sums(d.img, flags, rois, roi_flags)


ROIS = [{'type': 'text', 'bbox': [3, 2, 20, 12]}, {'type': 'product', 'bbox': [-4, -2, 20, 20]},
        {'type': 'face', 'bbox': [10, 5, 999, 999]}, {'type': 'brand', 'bbox': [1, 1, 9, 7], 'reference_color': (200, 30, 40)},
        {'type': 'brand', 'bbox': [1, 1, 9, 7]}, {'type': 'face', 'bbox': [2, 2, 0, 4]}, {'bbox': [0, 0, 5, 5]}, {'type': 'text'}]


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_key_order_values_and_json(cn):
    rng = np.random.default_rng(cn)
    img = rng.integers(0, 256, (23, 31) if cn == 1 else (23, 31, cn), dtype=np.uint8)
    got = _FakeQA().evaluate_commercial(img, ROIS)
    want = R.evaluate_commercial(img, ROIS)
    assert list(got) == list(want)
    assert list(got)[:2] == ['global_sharpness', 'high_frequency_ratio'] and list(got)[-1] == 'commercial_score'
    for k in want:
        assert type(got[k]) in (float, str), k
        if isinstance(want[k], str):
            assert got[k] == want[k]
        else:
            assert got[k] == pytest.approx(want[k], rel=R.tolerance(k), abs=1e-12), k
    assert json.loads(json.dumps(got)) == got
    if cn == 1:
        assert got['color_variance'] == 0.0 and got['face_naturalness_2'] == 50.0 and got['skin_tone_naturalness_2'] == 50.0
        assert got['brand_color_delta_e_3'] == 100.0 and got['brand_color_accuracy_3'] == 'poor'


def test_levels_and_commercial_score():
    q = qam.QualityAssessmentModule()
    assert [q._assess_niqe(v) for v in (3.0, 3.1, 5.0, 8.0, 8.1)] == ['excellent', 'good', 'good', 'fair', 'poor']
    assert [q._assess_brisque(v) for v in (20.0, 35.0, 50.0, 50.5)] == ['excellent', 'good', 'fair', 'poor']
    assert [q._assess_delta_e(v) for v in (1.0, 2.0, 5.0, 9.0)] == ['excellent', 'good', 'fair', 'poor']
    m = {'global_sharpness': 2000.0, 'high_frequency_ratio': 0.1, 'oversharpen_score': 80.0, 'artifact_score': 90.0}
    s = q._calculate_commercial_score(m)
    assert type(s) is float and s == (100 + 50 + 80 + 90) / 4
    assert q._calculate_commercial_score({}) == 50.0


def test_validation_before_any_device_call():
    q = _FakeQA()
    real = qam.QualityAssessmentModule()
    with pytest.raises(NotImplementedError):
        real.evaluate_commercial(np.full((8, 8, 3), 300, np.uint16))
    with pytest.raises(NotImplementedError):
        real.evaluate_no_reference(np.full((8, 8), 2.5, np.float32))
    with pytest.raises(ValueError):
        real.evaluate_commercial(np.zeros((8, 8, 2), np.uint8) + 9)
    with pytest.raises(ValueError):
        real.evaluate_commercial(np.zeros((4, 4, 4, 3), np.uint8) + 9)
    with pytest.raises(ValueError):
        real.evaluate_commercial(np.zeros((16, 16, 3), np.uint8) + 9, [{'type': 'text', 'bbox': [1, 2, 3]}])
    with pytest.raises(TypeError):
        real.evaluate_commercial(np.zeros((16, 16, 3), np.uint8) + 9, [{'type': 'text', 'bbox': [1.5, 2, 3, 4]}])
    with pytest.raises(ValueError):
        real.evaluate_commercial_device(0, (16, 16, 2))
    with pytest.raises(NotImplementedError):
        real.evaluate_commercial_device(0, (40000, 16, 3))
    assert q.calls == 0


def test_no_reference_finishing():
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (19, 27, 3), dtype=np.uint8)
    q = _FakeQA()
    ints, flts = _sums(img, 0)
    n = 19 * 27
    want = R.evaluate_no_reference(img)
    assert q._niqe_of(flts[0], n) == pytest.approx(want['niqe'], rel=1e-12)
    assert q._brisque_of(ints[0], flts[0], n) == pytest.approx(want['brisque'], rel=1e-12)
    assert q._colorfulness_of(ints[0], n) == pytest.approx(want['colorfulness'], rel=1e-12)


def test_kernel_gaussian_weights_are_the_restated_rule():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "super-resolution-system_amd", "csrc",
                            "sr_commercial.hip")).read()
    body = src[src.index("Gauss7 gauss7()"):src.index("int cm_workspace")]
    lits = [float.fromhex(v) for v in re.findall(r"(0x[0-9a-f.]+p-?\d+)f", body)]
    assert np.array_equal(np.array(lits, np.float32), R.gauss7_weights())


def test_native_table_lists_the_new_entry_points():
    for name in ("sr_commercial_u8", "sr_fft_c2c", "sr_fft_max_len"):
        assert name in _native.SIGNATURES
    assert qam._FFT_MAX_LEN == 32768
