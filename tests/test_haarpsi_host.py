"""CPU: the host side of HaarPSI (sr_haarpsi_plan, sr_haarpsi_value, sr_haarpsi_cell_value, the float64 restatement
sr_haarpsi_host_u8, every refusal of the entry points and of the module methods before a device call) and the NumPy / SciPy
restatement tests/_haarpsi_ref.py: both window conventions against convolve2d directly, the anchors of the definition, and
its mutants."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.signal import convolve2d

import _haarpsi_ref as H
import _native

TOL = 1e-12
CONVENTIONS = ("matlab", "python")


def _pair(rng, h, w, cn):
    a = rng.integers(0, 256, (h, w, cn), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-25, 26, a.shape), 0, 255).astype(np.uint8)
    return (a[..., 0].copy(), b[..., 0].copy()) if cn == 1 else (a, b)


def test_plan_sizes_and_counts():
    assert C.sizeof(_native.HaarPsiSums) == 64 and C.sizeof(_native.HaarPsiCell) == 16
    for h, w in ((2, 2), (5, 7), (41, 57), (42, 43), (97, 130), (67, 263)):
        for cb in (0, 1, 2, 3):
            for sub in (True, False):
                ch, cw = h - 2 * cb, w - 2 * cb
                if min(ch, cw) < 2:
                    with pytest.raises(_native.SrShapeError, match=r"at least 2\b"):
                        _native.haarpsi_plan(h, w, 3, cb, sub)
                    continue
                p = _native.haarpsi_plan(h, w, 3, cb, sub, "python")
                want = (-(-ch // 2), -(-cw // 2)) if sub else (ch, cw)
                assert p["size"] == want and p["count"] == want[0] * want[1]
                assert p["blocks"] == -(-want[0] // 16) * -(-want[1] // 64)
                assert 48 * p["blocks"] <= p["scratch_bytes"] <= 48 * p["blocks"] + 3 * 256 + (1 << 12)
    assert _native.load().sr_haarpsi_plan(64, 64, 3, 2, 1, 0, None, None, None, None, None) == _native.SR_OK    # outputs may be NULL


def test_plan_refusals():
    for kw, word in ((dict(cn=2), "channels"), (dict(cn=0), "channels"), (dict(convention=2), "convention"),
                     (dict(convention="piq"), "convention"), (dict(subsample=2), "subsample"), (dict(crop_border=-1), "crop_border"),
                     (dict(h=0), "h, w")):
        args = dict(h=64, w=64, cn=3, crop_border=2)
        args.update(kw)
        with pytest.raises(ValueError, match=word) as e:
            _native.haarpsi_plan(**args)
        assert not isinstance(e.value, _native.SrShapeError), kw
    for h, w, cb in ((1, 64, 0), (64, 1, 0), (7, 64, 3), (8, 8, 40)):
        with pytest.raises(_native.SrShapeError, match=r"at least 2\b"):
            _native.haarpsi_plan(h, w, 3, cb)
    _native.haarpsi_plan(8, 8, 4, 3)                                        # exactly 2 left


def test_value():
    x = 1.0 / (1.0 + math.exp(-4.2))
    assert _native.haarpsi_cell_value(0.5, 1.0) == 0.0
    assert _native.haarpsi_cell_value(x, 1.0) == pytest.approx(1.0, rel=TOL, abs=0)
    assert math.isnan(_native.haarpsi_cell_value(0.0, 0.0))
    assert _native.haarpsi_value({"num": [1.0, 2.0, 3.0], "den": [2.0, 4.0, 6.0]}) == 0.0
    assert _native.haarpsi_value({"num": [3.0 * x, x], "den": [3.0, 1.0]}) == pytest.approx(1.0, rel=TOL, abs=0)
    assert math.isnan(_native.haarpsi_value({"num": [0.0, 0.0], "den": [0.0, 0.0]}))
    with pytest.raises(ValueError, match="2 or 3 channels"):
        _native.haarpsi_value({"num": [1.0], "den": [1.0]})
    assert math.isnan(_native.load().sr_haarpsi_value(None))
    for q in (0.7, 0.9, 0.99):
        assert _native.haarpsi_cell_value(q, 1.0) == pytest.approx((math.log(q / (1 - q)) / 4.2) ** 2, rel=TOL, abs=0)


def test_host_restatement_matches_the_numpy_restatement():
    """The integer planes and direct window sums of the library against the float convolutions of the scripts: 1e-12 on
    every sum and on the value."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for h, w in ((2, 2), (2, 3), (3, 5), (7, 8), (16, 16), (17, 33), (33, 18), (37, 43)):
        for cn in (1, 3, 4):
            a, b = _pair(rng, h, w, cn)
            for conv in CONVENTIONS:
                for sub in (True, False):
                    for cb in (0, 1, 2):
                        if min(h, w) - 2 * cb < 2:
                            continue
                        want = H.haarpsi_ref(a, b, cb, sub, conv)
                        got = _native.haarpsi_host(a, b, cb, sub, conv)
                        assert got["channels"] == want["channels"] == (2 if cn == 1 else 3) and got["count"] == want["map_den"].size
                        v = _native.haarpsi_value(got)
                        for g, r in list(zip(got["num"], want["num"])) + list(zip(got["den"], want["den"])) + [(v, want["value"])]:
                            worst = max(worst, abs(g - r) / r)
                            assert g == pytest.approx(r, rel=TOL, abs=0), (h, w, cn, conv, sub, cb)
    print("largest relative distance", worst)
    # a strided view (rows of a wider array) is read in place
    wide = rng.integers(0, 256, (9, 40, 3), dtype=np.uint8)
    a, b = wide[:, 3:20], wide[:, 21:38]
    got, want = _native.haarpsi_host(a, b), H.haarpsi_ref(a, b)
    assert got["num"] == pytest.approx(want["num"], rel=TOL, abs=0)


def test_anchors():
    a, b = H.anchor_pair()
    assert a.shape == (17, 33, 3) and a[3, 5, 1] == (21 + 65 + 31 + 5 * (15 % 11)) % 256
    for (colour, conv, sub), want in H.ANCHORS.items():
        x, y = (a, b) if colour else (a[..., 0], b[..., 0])
        assert H.haarpsi_ref(x, y, 0, sub, conv)["value"] == pytest.approx(want, rel=TOL, abs=0), (colour, conv, sub)
        assert _native.haarpsi_value(_native.haarpsi_host(x, y, 0, sub, conv)) == pytest.approx(want, rel=TOL, abs=0)
    for rec in (H.haarpsi_ref(a, b), _native.haarpsi_host(a, b)):
        assert rec["num"] == pytest.approx(H.ANCHOR_NUM, rel=1e-11, abs=0)      # the definition quotes 12 digits
        assert rec["den"] == pytest.approx(H.ANCHOR_DEN, rel=1e-11, abs=0)


def test_properties_on_the_host():
    rng = np.random.default_rng(3)
    for cn in (1, 3):
        a, b = _pair(rng, 17, 22, cn)
        for conv in CONVENTIONS:
            for sub in (True, False):
                val = lambda x, y: _native.haarpsi_value(_native.haarpsi_host(x, y, 0, sub, conv))       # noqa: E731
                assert abs(val(a, a) - 1.0) <= 1e-12
                assert abs(val(a, b) - val(b, a)) <= 1e-12 and 0.0 < val(a, b) < 1.0
                z = np.zeros_like(a)
                assert math.isnan(val(z, z))
                f = np.full_like(a, 77)
                rec = _native.haarpsi_host(f, f, 0, sub, conv)
                assert rec["den"][0] > 0 and abs(_native.haarpsi_value(rec) - 1.0) <= 1e-12


def test_both_conventions_against_convolve2d():
    """'python' IS scipy's mode='same'; 'matlab' is the full convolution cropped at floor(k / 2): for an even kernel its
    window looks forward, one sample later than SciPy's; for an odd kernel the two agree."""
    x = np.random.default_rng(7).integers(0, 256, (9, 11)).astype(np.float64)
    for s in (1, 2, 3):
        for k in (H.haar_kernel(s), H.haar_kernel(s).T, np.ones((2, 2)) / 4.0):
            n = k.shape[0]
            assert np.array_equal(H.conv_same(x, k, "python"), convolve2d(x, k, mode="same"))
            full = convolve2d(x, k, mode="full")
            assert np.array_equal(H.conv_same(x, k, "matlab"), full[n // 2:n // 2 + 9, n // 2:n // 2 + 11])
            xp = np.pad(x, ((0, 1), (0, 1)))
            assert np.array_equal(H.conv_same(x, k, "matlab"), convolve2d(xp, k, mode="same")[1:, 1:])
    k3 = np.ones((3, 3))
    assert np.array_equal(H.conv_same(x, k3, "matlab"), H.conv_same(x, k3, "python"))
    xp = np.pad(x, ((0, 1), (0, 1)))
    assert np.array_equal(H.conv_same(x, np.ones((2, 2)), "matlab"), xp[:-1, :-1] + xp[1:, :-1] + xp[:-1, 1:] + xp[1:, 1:])
    xq = np.pad(x, ((1, 0), (1, 0)))
    assert np.array_equal(H.conv_same(x, np.ones((2, 2)), "python"), xq[:-1, :-1] + xq[1:, :-1] + xq[:-1, 1:] + xq[1:, 1:])
    # the library's integer windows are these: scale 1, rows above minus rows below at (i - o, j - o)
    a = np.random.default_rng(8).integers(0, 256, (6, 7), dtype=np.uint8)
    z = np.zeros_like(a)
    for conv in CONVENTIONS:
        v = np.abs(H.conv_same(a.astype(np.float64), H.haar_kernel(3), conv))
        rec = _native.haarpsi_host(a, z, 0, False, conv)                    # against black: w = the scale-3 coefficient of a
        assert rec["den"][0] == pytest.approx(v.sum(), rel=TOL, abs=0)
    va = _native.haarpsi_value
    assert abs(va(_native.haarpsi_host(a, a // 2, 0, True, "matlab")) - va(_native.haarpsi_host(a, a // 2, 0, True, "python"))) > 1e-4


@pytest.mark.parametrize("mutant", H.MUTANTS)
def test_restatement_kills_mutants(mutant):
    """Each plausible misreading of the definition moves the restatement's own answer by more than 1e-6."""
    rng = np.random.default_rng(23)
    a17, b17 = H.anchor_pair()
    for a, b in (_pair(rng, 33, 47, 3), (a17, b17)):
        for conv in CONVENTIONS:
            good, bad = H.haarpsi_ref(a, b, 0, True, conv)["value"], H.haarpsi_ref(a, b, 0, True, conv, mutant)["value"]
            print(mutant, a.shape, conv, good, bad, abs(bad - good))
            assert abs(bad - good) > 1e-6, (mutant, a.shape, conv)
            # ... and the library's restatement is the unmutated one
            assert _native.haarpsi_value(_native.haarpsi_host(a, b, 0, True, conv)) == pytest.approx(good, rel=TOL, abs=0)


def test_entry_points_refuse_before_any_device_call():
    lib = _native.load()
    out = _native.HaarPsiSums()
    cells = (_native.HaarPsiCell * 4)()
    buf = C.create_string_buffer(16)
    p = C.cast(buf, C.c_void_p)
    xe, ye = (C.c_int * 3)(0, 30, 56), (C.c_int * 3)(0, 5, 12)

    def call(a=p, sa=192, b=p, sb=192, h=20, w=64, cn=3, cb=4, sub=1, conv=0, o=C.byref(out)):
        rc = lib.sr_haarpsi_u8(None, a, sa, b, sb, h, w, cn, cb, sub, conv, o)
        return rc, _native.last_error()

    def call_cells(a=p, sa=192, b=p, sb=192, h=20, w=64, cn=3, cb=4, sub=1, conv=0, x=xe, gw=2, y=ye, gh=2, o=cells):
        rc = lib.sr_haarpsi_cells_u8(None, a, sa, b, sb, h, w, cn, cb, sub, conv, x, gw, y, gh, o)
        return rc, _native.last_error()

    for fn in (call, call_cells):
        for kw in (dict(), dict(conv=1), dict(sub=0), dict(cn=1, sa=64, sb=64), dict(cn=4, sa=256, sb=256), dict(h=10)):     # 10 - 8 = 2
            if fn is call_cells and "h" in kw:
                continue
            rc, msg = fn(**kw)
            assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg, (kw, msg)
        for kw in (dict(a=None), dict(b=None), dict(o=None)):
            rc, msg = fn(**kw)
            assert rc == _native.SR_ERR_INVALID_ARG and "null argument" in msg, kw
        for kw, word in ((dict(cn=2), "channels"), (dict(conv=2), "convention"), (dict(sub=2), "subsample"), (dict(cb=-1), "crop_border"),
                         (dict(h=0), "h, w")):
            rc, msg = fn(**kw)
            assert rc == _native.SR_ERR_INVALID_ARG and word in msg, (kw, msg)
        for kw, word in ((dict(sa=191), "stride"), (dict(sb=191), "stride"), (dict(h=9), "at least 2"), (dict(cb=32), "at least 2")):
            rc, msg = fn(**kw)
            assert rc == _native.SR_ERR_SHAPE and word in msg, (kw, msg)
    for kw, word in ((dict(x=(C.c_int * 3)(0, 30, 55)), "x edges"), (dict(y=(C.c_int * 3)(1, 5, 12)), "y edges"),
                     (dict(x=(C.c_int * 3)(0, 56, 56)), "strictly increasing"), (dict(gw=0), "at least one cell"), (dict(x=None), "null x")):
        rc, msg = call_cells(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and word in msg, (kw, msg)


def test_module_methods_refuse_before_any_device_call():
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()

    def no_device():
        raise AssertionError("the device context was asked for")
    q._ctx = no_device
    a = np.zeros((20, 64, 3), np.uint8)
    g = np.zeros((20, 64), np.uint8)
    for fn in (q.calculate_haarpsi, q.evaluate_haarpsi_map):
        with pytest.raises(NotImplementedError):
            fn(a.astype(np.float32), a)
        with pytest.raises(NotImplementedError):
            fn(a.astype(np.uint16), a.astype(np.uint16))
        for x, y in ((a, a[:19]), (a, g)):
            with pytest.raises(ValueError, match="same shape"):
                fn(x, y)
        with pytest.raises(ValueError, match="convention"):
            fn(a, a, convention="piq")
        with pytest.raises(ValueError, match="subsample"):
            fn(a, a, subsample=2)
        with pytest.raises(ValueError, match="1, 3 or 4 channels"):
            fn(a[..., :2], a[..., :2])
        with pytest.raises(AssertionError, match="device context"):
            fn(a, a)
    with pytest.raises(ValueError, match="at least 2"):
        q.calculate_haarpsi(a, a, crop_border=10)
    with pytest.raises(ValueError, match="crop_border"):
        q.calculate_haarpsi(a, a, crop_border=-1)
    with pytest.raises(ValueError, match="null"):
        q.calculate_haarpsi_device(256, (20, 64, 3), 0, (20, 64, 3))
    with pytest.raises(ValueError, match="null"):
        q.evaluate_haarpsi_map_device(0, (20, 64, 3), 256, (20, 64, 3))
    with pytest.raises(_native.SrShapeError, match="stride"):
        q.calculate_haarpsi_device(256, (20, 64, 3), 256, (20, 64, 3), stride1=100)
    with pytest.raises(ValueError, match="edges"):
        q.evaluate_haarpsi_map(a, a, x_edges=[0, 64])
    with pytest.raises(ValueError):
        q.evaluate_haarpsi_map(a, a, x_edges=[0, 63], y_edges=[0, 20])
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_haarpsi(a, a, crop_border=9)
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_haarpsi_device(256, (20, 64), 256, (20, 64), stride2=64)
    import main as sr_main
    assert sr_main.PipelineConfig().qa_haarpsi is False and sr_main.PipelineConfig(qa_haarpsi=True).qa_haarpsi is True
