"""CPU: the host side of the colour difference (sr_delta_e_plan, sr_delta_e_table, sr_delta_e_lab_u8, sr_delta_e_pair, the mean /
rms / percentile / fraction rules, every refusal of the two entry points and of the module methods before a device call) and
the NumPy restatement tests/_deltae_ref.py, both held to scikit-image 0.18.3's own values in tests/golden/deltae_skimage.npz at
1e-12 absolute; the restatement's mutants each leave that bar (and the 1e-9 bar of the GPU tests)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import _native
import _deltae_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deltae_skimage.npz")
TOL = 1e-12
FORMULAS = ((R.CIEDE2000, "de00"), (R.CIE76, "de76"))


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(GOLD))


def cases():
    return [str(c) for c in gold()["cases"]]


def test_fixture_meets_the_generator_conditions():
    g = gold()
    assert cases() == ["noisy", "rows", "primaries", "gray", "rgba"] and str(g["skimage_version"]) == "0.18.3"
    assert float(g["closest_to_pi"]) >= 1e-6 and float(g["closest_to_bin_edge"]) >= 1e-6
    assert int(g["wrap_counts"].min()) >= 10
    assert g["noisy_a"].shape == (60, 90, 3) and g["gray_a"].ndim == 2 and g["rgba_a"].shape[2] == 4
    for name in cases():                                  # (b), recomputed from the stored reference
        same = np.all(R.to_rgb(g[f"{name}_a"]) == R.to_rgb(g[f"{name}_b"]), axis=-1)
        for _, key in FORMULAS:
            d = g[f"{name}_{key}"]
            assert d.dtype == np.float64 and (d[same] == 0.0).all()
            nz = 16.0 * d[d != 0.0]
            assert np.abs(nz - np.round(nz)).min() >= 1e-6


def test_restatement_matches_scikit_image():
    g = gold()
    worst = 0.0
    for name in cases():
        a, b = g[f"{name}_a"], g[f"{name}_b"]
        worst = max(worst, float(np.abs(R.rgb2lab(a) - g[f"{name}_lab1"]).max()))
        for f, key in FORMULAS:
            worst = max(worst, float(np.abs(R.delta_e_map(a, b, f) - g[f"{name}_{key}"]).max()))
    for f, key in FORMULAS:
        got = R.pair(g["lab_pairs"][:, 0], g["lab_pairs"][:, 1], f)
        worst = max(worst, float(np.abs(got - g[f"lab_{key}"]).max()))
    print(f"restatement against scikit-image: largest distance {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_restatement_kills_mutants(mutant):
    """Each one-term error moves a value of the fixture (an image map or a constructed Lab pair) beyond 1e-9, the bar of the
    GPU tests, and so beyond the 1e-12 of this file."""
    g = gold()
    worst = 0.0
    for name in cases():
        worst = max(worst, float(np.abs(R.delta_e_map(g[f"{name}_a"], g[f"{name}_b"], R.CIEDE2000, mutant=mutant)
                                        - g[f"{name}_de00"]).max()))
    image_worst = worst
    got = R.pair(g["lab_pairs"][:, 0], g["lab_pairs"][:, 1], R.CIEDE2000, mutant)
    worst = max(worst, float(np.abs(got - g["lab_de00"]).max()))
    print(f"{mutant}: images {image_worst:.2e}, with the Lab pairs {worst:.2e}")
    assert worst > 1e-9
    if mutant != "nonstrict_pi":                          # condition (a) keeps every image pixel away from |h_diff| == pi
        assert image_worst > 1e-9


def test_native_lab_and_pair_match_scikit_image():
    g = gold()
    assert C.sizeof(_native.DeltaESums) == 32 + 8 * _native.DELTA_E_BINS and C.sizeof(_native.DeltaECell) == 16
    worst_lab = worst = 0.0
    for name in cases():
        a, b = R.to_rgb(g[f"{name}_a"]), R.to_rgb(g[f"{name}_b"])
        h, w = a.shape[:2]
        labs = {}
        for px in np.unique(np.concatenate([a.reshape(-1, 3), b.reshape(-1, 3)]), axis=0):
            labs[tuple(int(v) for v in px)] = _native.delta_e_lab(*[int(v) for v in px])
        la = np.array([[labs[tuple(int(v) for v in a[y, x])] for x in range(w)] for y in range(h)])
        worst_lab = max(worst_lab, float(np.abs(la - g[f"{name}_lab1"]).max()))
        for f, key in FORMULAS:
            want = g[f"{name}_{key}"]
            for y in range(h):
                for x in range(w):
                    got = _native.delta_e_pair(la[y, x], labs[tuple(int(v) for v in b[y, x])], f)
                    worst = max(worst, abs(got - want[y, x]))
    for f, key in FORMULAS:
        for p, want in zip(g["lab_pairs"], g[f"lab_{key}"]):
            worst = max(worst, abs(_native.delta_e_pair(p[0], p[1], f) - want))
    print(f"host functions against scikit-image: Lab {worst_lab:.2e}, dE {worst:.2e}")
    assert worst_lab <= TOL and worst <= TOL


def test_constructed_lab_pairs():
    # exactly at h_diff == pi with unequal chromas: the strict comparison decides; the non-strict reading is far away
    p1, p2 = (50.0, 10.0, 0.0), (50.0, -20.0, 0.0)
    strict = _native.delta_e_pair(p1, p2)
    assert strict == pytest.approx(float(R.ciede2000(np.array(p1), np.array(p2))), abs=TOL)
    assert abs(strict - float(R.ciede2000(np.array(p1), np.array(p2), mutant="nonstrict_pi"))) > 1e-3
    # equal chromas at h_diff == pi: no rotation term, both readings agree -- the pair the issue names
    e = _native.delta_e_pair((50.0, 10.0, 0.0), (50.0, -10.0, 0.0))
    assert e == pytest.approx(float(R.ciede2000(np.array((50.0, 10.0, 0.0)), np.array((50.0, -10.0, 0.0)))), abs=TOL) and e > 10
    # a zero chroma: the definition makes Hbar the SUM of the hues.  No input can tell: the hue term is 2 sqrt(0) sin(.) = 0
    # there and Hbar reaches the result only through it, so the halved reading gives the same bits
    for z1, z2 in (((50.0, 0.0, 0.0), (50.0, -10.0, -10.0)), ((30.0, 5.0, -40.0), (70.0, 0.0, 0.0)), ((50.0, 0.0, 0.0), (60.0, 0.0, 0.0))):
        got = _native.delta_e_pair(z1, z2)
        assert got == pytest.approx(float(R.ciede2000(np.array(z1), np.array(z2))), abs=TOL) and got > 1
        assert float(R.ciede2000(np.array(z1), np.array(z2))) == float(R.ciede2000(np.array(z1), np.array(z2), mutant="hbar_halved"))
    # equal triples are exactly 0; CIE76 is the Euclidean distance
    assert _native.delta_e_pair((41.0, 3.0, -8.0), (41.0, 3.0, -8.0)) == 0.0
    assert _native.delta_e_pair((50.0, 3.0, 4.0), (50.0, 0.0, 0.0), _native.DELTA_E_76) == 5.0
    # black is the only pixel without chroma; a gray pixel keeps a small one
    assert list(_native.delta_e_lab(0, 0, 0)) == [0.0, 0.0, 0.0]
    lab = _native.delta_e_lab(128, 128, 128)
    assert 0 < abs(lab[1]) < 1e-2 and 0 < abs(lab[2]) < 1e-2
    for bad in ((-1, 0, 0), (0, 256, 0)):
        with pytest.raises(ValueError, match="0 .. 255"):
            _native.delta_e_lab(*bad)
    with pytest.raises(_native.SrNativeError, match="formula"):
        _native.delta_e_pair(p1, p2, 2)
    with pytest.raises(ValueError, match="unknown formula"):
        _native.delta_e_pair(p1, p2, "cie94")


def test_table_is_numpys_within_one_ulp():
    t, want = _native.delta_e_table(), R.table()
    assert t[0] == 0.0 and t[255] == 1.0 and np.all(np.diff(t) > 0)
    assert np.all(np.abs(t - want) <= np.spacing(want))
    assert t[10] == (10 / 255.0) / 12.92 and t[11] > (11 / 255.0) / 12.92               # the two branches meet between 10 and 11


def test_plan():
    p = _native.delta_e_plan(97, 130, 3, 2)
    assert p["size"] == (93, 126) and p["count"] == 93 * 126 and p["blocks"] == 24          # 1 x ceil(93 / 4) tiles
    assert _native.delta_e_plan(1, 1, 1)["blocks"] == 1 and _native.delta_e_plan(3, 3, 4, 1)["count"] == 1
    assert _native.delta_e_plan(4, 256, 3)["blocks"] == 1 and _native.delta_e_plan(5, 256, 3)["blocks"] == 2
    assert _native.delta_e_plan(4, 257, 3)["blocks"] == 2
    # the launch stops growing at 2048 blocks: 2048 and 2049 tiles
    small, big = _native.delta_e_plan(4 * 2048, 5, 3), _native.delta_e_plan(4 * 2048 + 1, 5, 3)
    assert small["blocks"] == big["blocks"] == 2048 and small["scratch_bytes"] == big["scratch_bytes"]
    assert _native.delta_e_plan(97, 130, 3)["scratch_bytes"] < small["scratch_bytes"]
    assert _native.delta_e_plan(64, 64, 3, 0, "cie76") == _native.delta_e_plan(64, 64, 3, 0, _native.DELTA_E_2000)
    assert _native.load().sr_delta_e_plan(64, 64, 3, 2, 0, None, None, None, None, None) == _native.SR_OK   # outputs may be NULL
    for kw, word in ((dict(cn=2), "channels"), (dict(cn=0), "channels"), (dict(crop_border=-1), "crop_border"), (dict(h=0), "h, w")):
        args = dict(h=64, w=64, cn=3, crop_border=2)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            _native.delta_e_plan(**args)
    with pytest.raises(_native.SrShapeError, match="at least 1"):
        _native.delta_e_plan(8, 64, 3, 4)
    for f in (2, -1, 94):                                  # CIE94, CMC, other weights: refused by name
        with pytest.raises(_native.SrNativeError, match="CIE94"):
            _native.delta_e_plan(64, 64, 3, 0, f)


def _record(bins, sum_=0.0, sum2=0.0, mx=0.0):
    hist = np.zeros(_native.DELTA_E_BINS, np.uint64)
    for j, n in bins.items():
        hist[j] = n
    return {"count": int(hist.sum()), "sum": sum_, "sum2": sum2, "max": mx, "hist": hist}


def test_mean_rms_percentile_fraction_rules():
    rec = _record({0: 50, 16: 45, 48: 4, 2047: 1}, sum_=300.0, sum2=2500.0, mx=140.0)       # 100 pixels
    assert _native.delta_e_mean_rms(rec) == (3.0, 5.0)
    # k = max(1, ceil(p count / 100)) at the bin boundaries: pixels 1 .. 50 in bin 0, 51 .. 95 in bin 16, 96 .. 99 in bin 48
    for p, want in ((1e-9, 0.0), (1, 0.0), (50, 0.0), (50.000001, 1.0), (51, 1.0), (95, 1.0), (95.5, 3.0), (99, 3.0),
                    (99.0001, 2047 / 16.0), (100, 2047 / 16.0)):
        assert _native.delta_e_percentile(rec, p) == want == R.percentile(rec["hist"], rec["count"], p), p
    assert _native.delta_e_percentile(_record({0: 7}), 100) == 0.0                         # identical images
    assert _native.delta_e_percentile(_record({5: 1}), 0.5) == 5 / 16.0                     # one pixel: k = 1
    big = _record({3: 2 ** 40, 4: 1})                                                       # counts beyond 2^32
    assert _native.delta_e_percentile(big, 100) == 4 / 16.0 and _native.delta_e_percentile(big, 99.9999999) == 3 / 16.0
    for p in (0, -1, 100.0001, float("nan")):
        with pytest.raises(ValueError, match=r"\(0, 100\]"):
            _native.delta_e_percentile(rec, p)
    # fractions are exact at the bin edges: >= 0 is everything, the open last bin is >= 127.9375
    for t, want in ((0, 1.0), (0.0625, 0.5), (1, 0.5), (1.0625, 0.05), (3, 0.05), (3.0625, 0.01), (5, 0.01), (127.9375, 0.01)):
        assert _native.delta_e_fraction(rec, t) == want == R.fraction_at_least(rec["hist"], rec["count"], t), t
    for t in (0.1, 1.03, -0.0625, 128, 1e9, float("nan")):                                 # off the grid, or outside [0, 128)
        with pytest.raises(ValueError, match="multiple of 1/16"):
            _native.delta_e_fraction(rec, t)
    empty = _record({})
    for fn in (_native.delta_e_mean_rms, lambda r: _native.delta_e_percentile(r, 50), lambda r: _native.delta_e_fraction(r, 1)):
        with pytest.raises(ValueError, match="no pixel"):
            fn(empty)
    broken = dict(rec, count=99)
    with pytest.raises(ValueError, match="add up"):
        _native.delta_e_percentile(broken, 50)
    with pytest.raises(ValueError, match="add up"):
        _native.delta_e_fraction(broken, 1)
    lib = _native.load()
    assert lib.sr_delta_e_mean(None) != lib.sr_delta_e_mean(None) and "null record" in _native.last_error()
    assert lib.sr_delta_e_fraction_at_least(None, 1.0, None) == _native.SR_ERR_INVALID_ARG


def test_restatement_record_rules():
    d = np.array([[0.0, 0.0624999, 0.0625], [1.0, 127.99, 500.0]])
    s = R.sums(d)
    assert s["count"] == 6 and s["max"] == 500.0 and s["hist"][0] == 2 and s["hist"][1] == 1 and s["hist"][16] == 1
    assert s["hist"][2047] == 2 and int(s["hist"].sum()) == 6
    assert R.percentile(s["hist"], 6, 50) == 1 / 16.0 and R.fraction_at_least(s["hist"], 6, 1.0) == 0.5
    cs, cm = R.cells(d, [0, 1, 3], [0, 2])
    assert cs.tolist() == [[1.0, math.fsum([0.0624999, 0.0625, 127.99, 500.0])]] and cm.tolist() == [[1.0, 500.0]]


def test_entry_points_refuse_before_any_device_call():
    lib = _native.load()
    out = _native.DeltaESums()
    cell = (_native.DeltaECell * 4)()
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    xe, ye = (C.c_int * 3)(0, 30, 56), (C.c_int * 3)(0, 5, 12)

    def sums(a=p, sa=192, b=p, sb=192, h=20, w=64, cn=3, cb=4, f=0, m=None, ms=0, o=C.byref(out)):
        return lib.sr_delta_e_u8(None, a, sa, b, sb, h, w, cn, cb, f, m, ms, o), _native.last_error()

    def cells(a=p, sa=192, b=p, sb=192, h=20, w=64, cn=3, cb=4, f=0, x=xe, gw=2, y=ye, gh=2, o=cell):
        return lib.sr_delta_e_cells_u8(None, a, sa, b, sb, h, w, cn, cb, f, x, gw, y, gh, o), _native.last_error()

    for call in (sums, cells):
        for kw in (dict(), dict(f=1), dict(cn=1, sa=64, sb=64), dict(cn=4, sa=256, sb=256)):
            if call is cells and "cn" not in kw or call is sums:
                rc, msg = call(**kw)
                assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg, (call.__name__, kw, msg)
        for kw in (dict(a=None), dict(b=None), dict(o=None)):
            rc, msg = call(**kw)
            assert rc == _native.SR_ERR_INVALID_ARG and "null argument" in msg, kw
        for kw, word in ((dict(cn=2), "channels"), (dict(cb=-1), "crop_border"), (dict(h=0), "h, w")):
            rc, msg = call(**kw)
            assert rc == _native.SR_ERR_INVALID_ARG and word in msg, (kw, msg)
        for kw, word in ((dict(sa=191), "stride"), (dict(sb=191), "stride"), (dict(h=8), "at least 1"), (dict(cb=32), "at least 1")):
            rc, msg = call(**kw)
            assert rc == _native.SR_ERR_SHAPE and word in msg, (kw, msg)
        for f in (2, 3, -1):
            rc, msg = call(f=f)
            assert rc == _native.SR_ERR_UNSUPPORTED and "CIE94" in msg
    rc, msg = sums(cn=1, sa=64, sb=64)
    assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg
    # the optional map: 8-byte aligned, a stride that is a multiple of 8 and at least a cropped row (56 doubles)
    m8 = C.c_void_p(p.value + (8 - p.value % 8) % 8)
    assert sums(m=m8, ms=448)[1].count("context") == 1
    for kw, code, word in ((dict(m=C.c_void_p(m8.value + 4), ms=448), _native.SR_ERR_INVALID_ARG, "multiples of 8"),
                           (dict(m=m8, ms=452), _native.SR_ERR_INVALID_ARG, "multiples of 8"),
                           (dict(m=m8, ms=440), _native.SR_ERR_SHAPE, "map stride"), (dict(m=m8, ms=0), _native.SR_ERR_SHAPE, "map stride")):
        rc, msg = sums(**kw)
        assert rc == code and word in msg, (kw, msg)
    # the grid spans the CROPPED rectangle (56 x 12 here), strictly increasing
    for kw, word in ((dict(x=(C.c_int * 3)(0, 30, 64)), "cropped side"), (dict(y=(C.c_int * 3)(0, 5, 20)), "cropped side"),
                     (dict(x=(C.c_int * 3)(1, 30, 56)), "from 0"), (dict(x=(C.c_int * 3)(0, 56, 56)), "strictly increasing"),
                     (dict(y=(C.c_int * 3)(0, 12, 12)), "strictly increasing"), (dict(gw=0), "at least one cell"),
                     (dict(x=None), "null x edges"), (dict(y=None), "null y edges")):
        rc, msg = cells(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and word in msg, (kw, msg)


def test_cells_refuse_what_one_launch_does_not_cover():
    """A launch holds fewer than 2^32 threads along x, 2^24 - 1 blocks of 256: one block per cell and one per row chunk of at
    most 64 rows.  Beyond that the call is refused by name before the context is looked at (pointers are never followed)."""
    lib = _native.load()
    cell = (_native.DeltaECell * 1)()
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    cap = (1 << 24) - 1

    def cells(h, w, ye, gh, xe, gw):
        return lib.sr_delta_e_cells_u8(None, p, 3 * w, p, 3 * w, h, w, 3, 0, 0, xe, gw, ye, gh, cell), _native.last_error()

    one_x = (C.c_int * 2)(0, 1)
    rc, msg = cells(64 * cap, 1, (C.c_int * 2)(0, 64 * cap), 1, one_x, 1)                  # 2^24 - 1 chunks: goes on to the context
    assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg, msg
    rc, msg = cells(64 * cap + 1, 1, (C.c_int * 2)(0, 64 * cap + 1), 1, one_x, 1)          # one row more: 2^24 chunks
    assert rc == _native.SR_ERR_UNSUPPORTED and "row chunks" in msg and str(cap) in msg, msg
    ye = np.arange(4097, dtype=np.int32) * 2
    xe = np.arange(4097, dtype=np.int32) * 3
    ip = C.POINTER(C.c_int)
    rc, msg = cells(8192, 12288, ye.ctypes.data_as(ip), 4096, xe.ctypes.data_as(ip), 4096)  # 2^24 cells
    assert rc == _native.SR_ERR_UNSUPPORTED and "cells" in msg and str(cap) in msg, msg
    rc, msg = cells(8192, 12285, ye.ctypes.data_as(ip), 4096, xe[:4096].ctypes.data_as(ip), 4095)
    assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg, msg


def test_module_methods_refuse_before_any_device_call():
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()

    def no_device():
        raise AssertionError("the device context was asked for")
    q._ctx = no_device
    a = np.zeros((20, 64, 3), np.uint8)
    g = np.zeros((20, 64), np.uint8)
    for fn in (q.calculate_delta_e, q.evaluate_delta_e_map):
        with pytest.raises(NotImplementedError):
            fn(a.astype(np.float32), a)
        with pytest.raises(NotImplementedError):
            fn(a.astype(np.uint16), a.astype(np.uint16))
        for x, y in ((a, a[:19]), (a, a[:, :63]), (a, g), (a, np.zeros((20, 64, 4), np.uint8))):
            with pytest.raises(ValueError, match="same shape"):
                fn(x, y)
        with pytest.raises(ValueError, match="1, 3 or 4 channels"):
            fn(np.zeros((20, 64, 2), np.uint8), np.zeros((20, 64, 2), np.uint8))
        for f in ("cie94", "cmc", "CIEDE2000", 2):
            with pytest.raises(ValueError, match="formula"):
                fn(a, a, formula=f)
    with pytest.raises(ValueError, match="crop_border"):
        q.calculate_delta_e(a, a, crop_border=-1)
    with pytest.raises(ValueError, match="at least 1"):
        q.calculate_delta_e(a, a, crop_border=10)
    for ps in ((0,), (50, 101), (-5,)):
        with pytest.raises(ValueError, match="percentiles"):
            q.calculate_delta_e(a, a, percentiles=ps)
    with pytest.raises(ValueError, match="null"):
        q.calculate_delta_e_device(256, (20, 64, 3), 0, (20, 64, 3))
    with pytest.raises(ValueError, match="null"):
        q.evaluate_delta_e_map_device(0, (20, 64, 3), 256, (20, 64, 3))
    with pytest.raises(_native.SrShapeError, match="stride"):
        q.calculate_delta_e_device(256, (20, 64, 3), 256, (20, 64, 3), stride1=100)
    # the argument rules of evaluate_quality_map
    with pytest.raises(ValueError, match="both x_edges and y_edges"):
        q.evaluate_delta_e_map(a, a, x_edges=[0, 64])
    with pytest.raises(ValueError, match="either cell or the edge lists"):
        q.evaluate_delta_e_map(a, a, cell=8, x_edges=[0, 64], y_edges=[0, 20])
    with pytest.raises(ValueError, match="cell must be"):
        q.evaluate_delta_e_map(a, a, cell=0)
    with pytest.raises(ValueError, match="strictly increasing"):
        q.evaluate_delta_e_map(a, a, x_edges=[0, 64, 64], y_edges=[0, 20])
    with pytest.raises(ValueError, match="from 0 to"):
        q.evaluate_delta_e_map(a, a, x_edges=[0, 60], y_edges=[0, 20])
    for fn, args in ((q.calculate_delta_e, (a, a)), (q.calculate_delta_e, (g, g)), (q.evaluate_delta_e_map, (a, a))):
        with pytest.raises(AssertionError, match="device context"):
            fn(*args)
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_delta_e_device(256, (20, 64, 4), 256, (20, 64, 4), stride2=256, formula="cie76")
    # the private brand-colour path keeps its name and its keys: a different quantity
    assert hasattr(q, "_calculate_delta_e") and "MEAN" in q.calculate_delta_e.__doc__


def test_pipeline_switch_is_off_by_default():
    import main as sr_main
    cfg = sr_main.PipelineConfig()
    assert cfg.qa_delta_e is False
    assert sr_main.PipelineConfig(qa_delta_e=True).qa_delta_e is True
