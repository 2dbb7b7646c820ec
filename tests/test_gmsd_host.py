"""CPU: the host side of GMSD (sr_gmsd_plan, sr_gmsd_value, every refusal of sr_gmsd_u8 and of the module methods before a
device call) and the NumPy / SciPy restatement tests/_gmsd_ref.py: MATLAB's 'same' for the even kernel, its mutants."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.signal import convolve2d

import _gmsd_ref as G
import _native
import _vif_ref as R


def test_plan_sizes_and_counts_against_the_restatement():
    assert C.sizeof(_native.GmsdSums) == 24
    rng = np.random.default_rng(9)
    for h, w in ((4, 4), (5, 7), (41, 57), (42, 43), (97, 130)):
        for cb in (0, 1, 2, 3):
            ch, cw = h - 2 * cb, w - 2 * cb
            if min(ch, cw) < 4:
                with pytest.raises(_native.SrShapeError, match=r"at least 4\b"):
                    _native.gmsd_plan(h, w, 1, cb, R.CHANNELS)
                continue
            p = _native.gmsd_plan(h, w, 1, cb, R.CHANNELS)
            assert p["size"] == (-(-ch // 2), -(-cw // 2)) and p["count"] == p["size"][0] * p["size"][1]
            a, b = R.img_pair(rng, h, w, 1)
            r = G.gmsd(a, b, cb, R.CHANNELS)
            assert r["q"].shape == p["size"] and r["count"] == p["count"]
            tiles = -(-p["size"][0] // 16) * -(-p["size"][1] // 64)
            assert 16 * tiles <= p["scratch_bytes"] <= 16 * tiles + 3 * 256 + (1 << 12)
    assert _native.load().sr_gmsd_plan(64, 64, 3, 2, 1, None, None, None, None) == _native.SR_OK            # outputs may be NULL


def test_plan_refusals():
    for kw, word in ((dict(cn=2), "channels"), (dict(cn=0), "channels"), (dict(mode=3), "mode"), (dict(cn=1, mode=R.Y), "Y modes"),
                     (dict(cn=3, mode=R.CHANNELS), "one gray plane"), (dict(crop_border=-1), "crop_border"), (dict(h=0), "h, w")):
        args = dict(h=64, w=64, cn=3, crop_border=2, mode=R.Y)
        args.update(kw)
        with pytest.raises(ValueError, match=word) as e:
            _native.gmsd_plan(**args)
        assert not isinstance(e.value, _native.SrShapeError), kw
    for h, w, cb in ((3, 64, 0), (64, 3, 0), (9, 64, 3), (8, 8, 40)):
        with pytest.raises(_native.SrShapeError, match=r"at least 4\b"):
            _native.gmsd_plan(h, w, 3, cb)
    _native.gmsd_plan(10, 10, 3, 3)                                         # exactly 4 left


def test_value():
    assert _native.gmsd_value({"sum_d": 6.0, "sum_d2": 14.0, "count": 3}) == 1.0          # d = 1, 2, 3
    assert _native.gmsd_value({"sum_d": 3.0, "sum_d2": 3.0, "count": 3}) == 0.0
    assert _native.gmsd_value({"sum_d": 3.0, "sum_d2": 3.0 - 1e-15, "count": 3}) == 0.0    # rounding below 0 is 0, not NaN
    with pytest.raises(ValueError, match="at least 2"):
        _native.gmsd_value({"sum_d": 1.0, "sum_d2": 1.0, "count": 1})
    assert math.isnan(_native.load().sr_gmsd_value(None))
    # the record's sums of d = 1 - q give the deviation of q
    a, b = R.img_pair(np.random.default_rng(2), 33, 47, 3)
    r = G.gmsd(a, b)
    assert _native.gmsd_value(r) == pytest.approx(r["score"], rel=1e-12, abs=0) and 0.001 < r["score"] < 0.5


def test_entry_point_refuses_before_any_device_call():
    lib = _native.load()
    out = _native.GmsdSums()
    buf = C.create_string_buffer(16)
    p = C.cast(buf, C.c_void_p)

    def call(a=p, sa=192, b=p, sb=192, h=20, w=64, cn=3, cb=4, mode=R.Y, o=C.byref(out)):
        rc = lib.sr_gmsd_u8(None, a, sa, b, sb, h, w, cn, cb, mode, o)
        return rc, _native.last_error()

    for kw in (dict(), dict(mode=R.Y_ROUND), dict(cn=1, sa=64, sb=64, mode=R.CHANNELS), dict(h=12)):     # 12 - 8 = 4: fine
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg, kw
    for kw in (dict(a=None), dict(b=None), dict(o=None)):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and "null argument" in msg, kw
    for kw, word in ((dict(cn=2), "channels"), (dict(cn=1, sa=64, sb=64), "Y modes"), (dict(mode=R.CHANNELS), "one gray plane"),
                     (dict(mode=3), "mode"), (dict(cb=-1), "crop_border"), (dict(h=0), "h, w")):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and word in msg, (kw, msg)
    for kw, word in ((dict(sa=191), "stride"), (dict(sb=191), "stride"), (dict(h=11), "at least 4"), (dict(cb=31), "at least 4")):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_SHAPE and word in msg, (kw, msg)


def test_module_methods_refuse_before_any_device_call():
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()

    def no_device():
        raise AssertionError("the device context was asked for")
    q._ctx = no_device
    a = np.zeros((20, 64, 3), np.uint8)
    g = np.zeros((20, 64), np.uint8)
    with pytest.raises(NotImplementedError):
        q.calculate_gmsd(a.astype(np.float32), a)
    for x, y in ((a, a[:19]), (a, g)):
        with pytest.raises(ValueError, match="same shape"):
            q.calculate_gmsd(x, y)
    with pytest.raises(ValueError, match="luma only"):
        q.calculate_gmsd(a, a, test_y_channel=False)
    with pytest.raises(ValueError, match="y_round"):
        q.calculate_gmsd(g, g, y_round=True)
    with pytest.raises(ValueError, match="at least 4"):
        q.calculate_gmsd(a, a, crop_border=9)
    with pytest.raises(ValueError, match="null"):
        q.calculate_gmsd_device(256, (20, 64, 3), 0, (20, 64, 3))
    with pytest.raises(_native.SrShapeError, match="stride"):
        q.calculate_gmsd_device(256, (20, 64, 3), 256, (20, 64, 3), stride1=100)
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_gmsd(a, a, crop_border=8)
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_gmsd_device(256, (20, 64), 256, (20, 64), stride2=64)


def test_matlab_same_for_the_even_kernel():
    """conv2(P, ones(2) / 4, 'same') is the mean of P(i .. i + 1, j .. j + 1) with zero beyond the last row and column; for the
    odd Prewitt kernels 'same' is SciPy's."""
    x = np.random.default_rng(7).integers(0, 256, (6, 7)).astype(np.float64)
    xp = np.pad(x, ((0, 1), (0, 1)))
    assert np.array_equal(G.conv_same(x, np.ones((2, 2)) / 4.0), (xp[:-1, :-1] + xp[1:, :-1] + xp[:-1, 1:] + xp[1:, 1:]) / 4.0)
    k3 = np.array([[1.0, 0.0, -1.0]] * 3) / 3.0
    for k in (k3, k3.T):
        assert np.array_equal(G.conv_same(x, k), convolve2d(x, k, mode="same"))
    xe = np.pad(x, ((0, 1), (0, 1)), mode="edge")
    assert np.array_equal(G.conv_same(x, np.ones((2, 2)) / 4.0, True), (xe[:-1, :-1] + xe[1:, :-1] + xe[:-1, 1:] + xe[1:, 1:]) / 4.0)
    # identical images: exactly 0
    u = x.astype(np.uint8)
    assert G.gmsd(u, u, 0, R.CHANNELS)["score"] == 0.0


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_restatement_kills_mutants(mutant):
    """Each plausible misreading of the definition moves the restatement's own answer by more than 1e-6 relative."""
    rng = np.random.default_rng(23)
    for h, w in ((33, 47), (97, 130)):
        a, b = R.img_pair(rng, h, w, 3)
        good, bad = G.gmsd(a, b)["score"], G.gmsd(a, b, mutant=mutant)["score"]
        rel = abs(bad - good) / good
        print(mutant, h, w, good, bad, rel)
        assert rel > 1e-6, (mutant, h, w)
