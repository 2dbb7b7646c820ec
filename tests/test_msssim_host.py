"""CPU: the host side of the multi-scale SSIM (sr_ms_ssim_plan, sr_ms_ssim_value, every refusal of sr_ms_ssim_u8 and of the
module methods before a device call) and the NumPy restatement tests/_msssim_ref.py against the two scikit-image fixtures."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _msssim_ref as R
import _native

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_plan_sizes_counts_and_refusals():
    for h, w in ((176, 176), (177, 191), (191, 353), (300, 600), (1000, 177), (11550, 17320)):
        for levels in range(1, 6):
            sizes, counts = R.plan(h, w, levels)
            p = _native.ms_ssim_plan(h, w, levels)
            assert p["sizes"] == sizes and p["counts"] == counts, (h, w, levels)
            # the planes of levels 1 .. L-1 as 4-byte pairs of 16-bit sums, plus small partial buffers
            planes = sum(a * b * 4 for a, b in sizes[1:])
            assert planes <= p["scratch_bytes"] <= planes + (1 << 20) + 256 * levels, (h, w, levels)
    assert _native.ms_ssim_plan(176, 176, 5)["sizes"][4] == (11, 11) and _native.ms_ssim_plan(176, 176, 5)["counts"][4] == 1
    big = _native.ms_ssim_plan(11550, 17320, 5)
    assert big["scratch_bytes"] < 11550 * 17320 * 4 // 3 + (1 << 20)    # about M / 3 * 4 bytes
    for levels in (0, 6, -1):
        with pytest.raises(ValueError, match="levels"):
            _native.ms_ssim_plan(512, 512, levels)
    with pytest.raises(ValueError):
        _native.ms_ssim_plan(512, 512, 2.5)
    for levels in range(1, 6):
        need = 11 << (levels - 1)
        _native.ms_ssim_plan(need, need, levels)
        for h, w in ((need - 1, need), (need, need - 1), (need - 1, 4000)):
            with pytest.raises(_native.SrShapeError, match=rf"at least {need}\b"):       # the minimum is named
                _native.ms_ssim_plan(h, w, levels)
            with pytest.raises(ValueError):
                R.plan(h, w, levels)
    with pytest.raises(ValueError):
        _native.ms_ssim_plan(0, 100, 1)
    lib = _native.load()
    assert lib.sr_ms_ssim_plan(176, 176, 5, None, None, None, None) == _native.SR_OK                 # outputs may be NULL


def test_value_formula():
    rnd = np.random.default_rng(3)
    for levels in range(1, 6):
        cnt = [int(rnd.integers(1, 10 ** 6)) for _ in range(levels)]
        s = [float(rnd.uniform(0.05, 1.0)) for _ in range(levels)]
        cs = [float(rnd.uniform(0.05, 1.0)) for _ in range(levels)]
        recs = [(s[j] * cnt[j], cs[j] * cnt[j], cnt[j]) for j in range(levels)]
        sm, csm = [r[0] / r[2] for r in recs], [r[1] / r[2] for r in recs]
        assert _native.ms_ssim_value(recs) == pytest.approx(R.value(sm, csm), rel=1e-15)
        wt = [float(v) for v in rnd.uniform(0.1, 2.0, levels)]
        assert _native.ms_ssim_value(recs, wt) == pytest.approx(R.value(sm, csm, wt), rel=1e-15)
        assert _native.ms_ssim_value(recs, wt) != _native.ms_ssim_value(recs)
        with pytest.raises(ValueError, match="weights"):
            _native.ms_ssim_value(recs, wt + [1.0])
    # the last level contributes S, the others CS
    recs = [(0.5 * 10, 0.9 * 10, 10), (0.25 * 7, 0.8 * 7, 7)]
    assert _native.ms_ssim_value(recs, (1.0, 1.0)) == pytest.approx(0.9 * 0.25, rel=1e-15)
    assert _native.ms_ssim_value(recs[:1], (1.0,)) == pytest.approx(0.5, rel=1e-15)
    assert _native.ms_ssim_value(recs) == pytest.approx(0.9 ** 0.0448 * 0.25 ** 0.2856, rel=1e-15)
    # a negative mean clamps to 0: the product is exactly 0.0, whichever level it is
    assert _native.ms_ssim_value([(0.5, -0.3, 1), (0.7, 0.9, 1)]) == 0.0
    assert _native.ms_ssim_value([(0.5, 0.3, 1), (-0.7, 0.9, 1)]) == 0.0
    assert _native.ms_ssim_value([(-0.5, 0.3, 1), (0.7, -0.9, 1)]) > 0.0             # unused terms may be negative
    assert R.value([0.5, -0.7], [0.3, 0.9]) == 0.0
    with pytest.raises(ValueError):
        _native.ms_ssim_value([])
    with pytest.raises(ValueError):
        _native.ms_ssim_value([(1.0, 1.0, 1)] * 6)
    with pytest.raises(ValueError):
        _native.ms_ssim_value([(1.0, 1.0, 0)])
    with pytest.raises(ValueError):
        _native.ms_ssim_value([(1.0, 1.0, 1)], (float("nan"),))
    lib = _native.load()
    assert math.isnan(lib.sr_ms_ssim_value(None, 1, None))
    one = (_native.MsSsimLevel * 1)(_native.MsSsimLevel(1.0, 1.0, 0))
    assert math.isnan(lib.sr_ms_ssim_value(one, 1, None)) and math.isnan(lib.sr_ms_ssim_value(one, 0, None))


def test_entry_point_refuses_before_any_device_call():
    """With a null context every valid argument list ends in 'null or destroyed context'; every refusal below comes first."""
    lib = _native.load()
    out = (_native.MsSsimLevel * 5)()
    buf = C.create_string_buffer(16)
    p = C.cast(buf, C.c_void_p)

    def call(a=p, sa=600, b=p, sb=600, h=176, w=200, cn=3, shift=15, dr=255.0, levels=5, o=out):
        rc = lib.sr_ms_ssim_u8(None, a, sa, b, sb, h, w, cn, shift, dr, levels, o)
        return rc, _native.last_error()

    rc, msg = call()
    assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg
    for kw in (dict(a=None), dict(b=None), dict(o=None)):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and "null argument" in msg, kw
    for kw, word in ((dict(cn=2), "channels"), (dict(cn=4), "channels"), (dict(shift=13), "gray_shift"), (dict(shift=16), "gray_shift"),
                     (dict(dr=0.0), "data_range"), (dict(dr=-1.0), "data_range"), (dict(dr=float("inf")), "data_range"),
                     (dict(dr=float("nan")), "data_range"), (dict(levels=0), "levels"), (dict(levels=6), "levels"),
                     (dict(h=0), "h, w")):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and word in msg, (kw, msg)
    for kw, word in ((dict(sa=599), "stride"), (dict(sb=599), "stride"), (dict(cn=1, sa=199), "stride"), (dict(h=175), "at least 176"),
                     (dict(w=175, sa=525, sb=525), "at least 176"), (dict(h=87, levels=4), "at least 88")):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_SHAPE and word in msg, (kw, msg)
    rc, msg = call(h=87, levels=3)
    assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg              # 87 >= 44: fine for three levels
    assert lib.sr_ms_ssim_planes(None, 1, p, p) == _native.SR_ERR_INVALID_ARG and "context" in _native.last_error()
    assert lib.sr_ms_ssim_planes(None, 1, None, p) == _native.SR_ERR_INVALID_ARG and "null argument" in _native.last_error()


def test_module_methods_refuse_before_any_device_call():
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()

    def no_device():
        raise AssertionError("the device context was asked for")
    q._ctx = no_device
    a = np.zeros((200, 180, 3), np.uint8)
    g = np.zeros((200, 180), np.uint8)
    with pytest.raises(NotImplementedError):                                 # float data with max > 1 stays float
        q.calculate_ms_ssim(a.astype(np.float32) + 7.0, a)
    with pytest.raises(NotImplementedError):
        q.calculate_ms_ssim(g, g.astype(np.uint16) + 300)
    with pytest.raises(ValueError, match="channel layouts"):
        q.calculate_ms_ssim(a, g)
    with pytest.raises(ValueError, match="3 channels"):
        q.calculate_ms_ssim(np.zeros((200, 180, 4), np.uint8), np.zeros((200, 180, 4), np.uint8))
    with pytest.raises(ValueError, match="at least 176"):
        q.calculate_ms_ssim(a[:175], a)                                      # the common rectangle is 175 rows
    with pytest.raises(ValueError, match="at least 176"):
        q.calculate_ms_ssim(g[:, :100], g[:, :100])
    for levels in (0, 6, 2.5):
        with pytest.raises(ValueError):
            q.calculate_ms_ssim(a, a, levels=levels)
    with pytest.raises(ValueError, match="weights"):
        q.calculate_ms_ssim(a, a, weights=(0.5, 0.5))
    with pytest.raises(ValueError, match="weights"):
        q.calculate_ms_ssim(a, a, levels=2, weights=(0.5, float("inf")))
    for dr in (0.0, -255.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="data_range"):
            q.calculate_ms_ssim(a, a, data_range=dr)
    # the device form
    with pytest.raises(ValueError, match="channel layouts"):
        q.calculate_ms_ssim_device(256, (200, 180, 3), 256, (200, 180))
    with pytest.raises(ValueError, match="3 channels"):
        q.calculate_ms_ssim_device(256, (200, 180, 2), 256, (200, 180, 2))
    with pytest.raises(ValueError, match="null"):
        q.calculate_ms_ssim_device(0, (200, 180, 3), 256, (200, 180, 3))
    with pytest.raises(ValueError, match="at least 176"):
        q.calculate_ms_ssim_device(256, (200, 180, 3), 256, (100, 180, 3))
    with pytest.raises(ValueError, match="levels"):
        q.calculate_ms_ssim_device(256, (200, 180, 3), 256, (200, 180, 3), levels=7)
    # a valid call gets as far as the context, and no further
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_ms_ssim(a, a)
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_ms_ssim_device(256, (200, 180), 256, (200, 180), levels=3, weights=(1, 1, 1))
    # the pipeline option is off by default
    import main as sr_main
    assert sr_main.PipelineConfig().qa_ms_ssim is False


def test_restatement_level_0_is_the_skimage_gaussian_ssim():
    z = np.load(os.path.join(GOLD, "metrics_skimage.npz"))
    assert len(z["cases"]) == 3
    for name in z["cases"]:
        a, b = np.ascontiguousarray(z[f"{name}_a"][..., 1]), np.ascontiguousarray(z[f"{name}_b"][..., 1])
        v, s, cs = R.ms_ssim(a, b, levels=1, weights=(1.0,))
        print(name, v, float(z[f"{name}_ssim_gauss"]), v - float(z[f"{name}_ssim_gauss"]))
        assert v == s[0] == float(z[f"{name}_ssim_gauss"])


def test_restatement_levels_match_skimage_on_the_pooled_planes():
    z = np.load(os.path.join(GOLD, "msssim_skimage.npz"))
    a, b = z["a"], z["b"]
    assert a.shape == b.shape == (177, 191) and a.dtype == np.uint8 and str(z["skimage_version"]) == "0.18.3"
    v, s, cs = R.ms_ssim(a, b)
    print("S", s, "CS", cs, "skimage", z["s"].tolist(), "value", v)
    assert len(z["s"]) == 5
    for j in range(5):
        assert abs(s[j] - float(z["s"][j])) <= 1e-12, j
    # the stored pair is what the input maker gives, and it separates the levels
    a2, b2 = R.img_pair(np.random.default_rng(20260313), 177, 191)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)
    assert all(1 - c >= 0.05 for c in cs) and all(abs(x - y) >= 1e-5 for x, y in zip(s, cs))
    # exact pooling: integer sums of 4^j values, odd last row / column dropped
    sums = R.pool_sums(a, 5)
    assert [p.shape for p in sums] == [(177, 191), (88, 95), (44, 47), (22, 23), (11, 11)]
    assert sums[4][0, 0] == int(a[:16, :16].astype(np.int64).sum()) and sums[1][-1, -1] == int(a[174:176, 188:190].astype(np.int64).sum())
    assert max(int(p.max()) for p in sums) <= 65280
