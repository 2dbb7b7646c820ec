"""CPU: the host side of VIF (sr_vif_plan, sr_vif_window, sr_vif_value, every refusal of sr_vif_u8 and of the module methods
before a device call, the pipeline option's default) and the NumPy / SciPy restatement tests/_vif_ref.py: its sizes against
the plan, its mutants."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _native
import _vif_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_records_and_the_header():
    assert (R.CHANNELS, R.Y, R.Y_ROUND) == (_native.BENCH_CHANNELS, _native.BENCH_Y, _native.BENCH_Y_ROUND)
    assert C.sizeof(_native.VifScale) == 24 and _native.VIF_SCALES == R.SCALES == 4
    text = open(os.path.join(ROOT, "include", "sr_hip.h")).read()
    assert "typedef struct sr_vif_scale" in text and "vifp_mscale" in text
    # the contract's words on parity stand in the header and the README
    assert "PARITY UNPINNED for both" in text and "N - 1" in text and "gaussian_filter" in text
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "vifp_mscale" in readme and "GMSD" in readme and "unpinned" in readme.lower()


# 41: one sample at scale 4; 42, 43 and the crops change the parity of H - 8 (and of the sizes below it)
SHAPES = [(41, 41), (41, 57), (42, 43), (97, 130)]


def test_plan_sizes_and_counts_against_the_restatement():
    rng = np.random.default_rng(5)
    for h, w in SHAPES + [(47, 48), (48, 49)]:
        for cb in (0, 1, 2, 3):
            ch, cw = h - 2 * cb, w - 2 * cb
            if min(ch, cw) < 41:
                with pytest.raises(_native.SrShapeError, match=r"at least 41\b"):
                    _native.vif_plan(h, w, 1, cb, R.CHANNELS)
                with pytest.raises(ValueError):
                    R.plan_sizes(h, w, cb)
                continue
            p = _native.vif_plan(h, w, 1, cb, R.CHANNELS)
            sizes, counts = R.plan_sizes(h, w, cb)
            assert p["sizes"] == sizes and p["counts"] == counts, (h, w, cb)
            assert p["sizes"][0] == (ch, cw) and p["counts"][0] == (ch - 16) * (cw - 16)
            assert p == {**_native.vif_plan(h, w, 3, cb, R.Y), "scratch_bytes": p["scratch_bytes"]}
            # the array shapes of the restatement itself
            a, b = R.img_pair(rng, h, w, 1)
            r = R.vifp(a, b, cb, R.CHANNELS)
            assert [tuple(s) for s in r["sizes"]] == sizes and r["count"] == counts, (h, w, cb)
            assert [(s[0] - R.taps(k + 1) + 1, s[1] - R.taps(k + 1) + 1) for k, s in enumerate(sizes)] == [tuple(m) for m in r["maps"]]
            # three pairs of float64 planes, two doubles per block, small reduction buffers
            planes = sum(2 * 8 * s[0] * s[1] for s in sizes[1:])
            assert planes <= p["scratch_bytes"] <= planes + 9 * 256 + 16 * (counts[0] // 16 + 64) + (1 << 12), (h, w, cb, p)
    assert _native.vif_plan(41, 41, 3)["counts"] == [625, 81, 9, 1]
    assert _native.vif_plan(41, 41, 3)["sizes"] == [(41, 41), (17, 17), (7, 7), (3, 3)]
    # the parity of H - 8: 49 -> ceil(41 / 2) = 21, 50 -> 21, 51 -> 22
    assert [_native.vif_plan(h, 60, 3)["sizes"][1][0] for h in (49, 50, 51)] == [21, 21, 22]
    big = _native.vif_plan(11550, 17320, 3)
    assert big["sizes"][0] == (11550, 17320) and big["sizes"][1] == (5771, 8656) and big["counts"][0] == 11534 * 17304
    assert _native.load().sr_vif_plan(64, 64, 3, 2, 1, None, None, None, None) == _native.SR_OK            # outputs may be NULL


def test_the_minimum_is_41():
    for h, w, cb in ((40, 64, 0), (64, 40, 0), (46, 64, 3), (64, 46, 3), (8, 8, 4), (8, 8, 40)):
        with pytest.raises(_native.SrShapeError, match=r"at least 41\b"):
            _native.vif_plan(h, w, 3, cb)
    _native.vif_plan(41, 41, 3)
    _native.vif_plan(47, 47, 3, 3)                                          # exactly 41 left
    with pytest.raises(ValueError, match="at least 41"):
        R.vifp(np.zeros((40, 41), np.uint8), np.zeros((40, 41), np.uint8), 0, R.CHANNELS)


def test_plan_refusals():
    for kw, word in ((dict(cn=2), "channels"), (dict(cn=4), "channels"), (dict(cn=0), "channels"), (dict(mode=3), "mode"),
                     (dict(mode=-1), "mode"), (dict(cn=1, mode=R.Y), "Y modes"), (dict(cn=1, mode=R.Y_ROUND), "Y modes"),
                     (dict(cn=3, mode=R.CHANNELS), "one gray plane"), (dict(crop_border=-1), "crop_border"), (dict(h=0), "h, w"),
                     (dict(w=-5), "h, w")):
        args = dict(h=64, w=64, cn=3, crop_border=2, mode=R.Y)
        args.update(kw)
        with pytest.raises(ValueError, match=word) as e:
            _native.vif_plan(**args)
        assert not isinstance(e.value, _native.SrShapeError), kw
    with pytest.raises(ValueError):
        _native.vif_plan(64, 64, 3, 1.5)


def test_window_is_fspecial():
    for scale in (1, 2, 3, 4):
        n = R.taps(scale)
        t = _native.vif_window(scale)
        assert t.shape == (n,) and n == (17, 9, 5, 3)[scale - 1]
        w2 = R.window(scale)
        assert w2.shape == (n, n) and np.all(w2 > 0)                         # the eps truncation never bites
        err = np.abs(np.outer(t, t) - w2).max()
        print(scale, n, err)
        assert err <= 1e-15
        assert abs(t.sum() - 1.0) <= 1e-15 and np.array_equal(t, t[::-1])
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match="scale"):
            _native.vif_window(bad)


def test_value():
    rec = [(1.0, 2.0, 10), (2.0, 3.0, 10), (3.0, 4.0, 10), (4.0, 5.0, 10)]
    assert _native.vif_value(rec) == 10.0 / 14.0
    assert math.isnan(_native.vif_value([(0.0, 0.0, 10)] * 4))               # a flat reference: MATLAB's 0 / 0
    with pytest.raises(ValueError, match="4 scale"):
        _native.vif_value(rec[:3])
    lib = _native.load()
    assert math.isnan(lib.sr_vif_value(None, 4)) and "scale records" in _native.last_error()
    arr = (_native.VifScale * 4)()
    assert math.isnan(lib.sr_vif_value(arr, 5))
    # the restatement on a flat reference
    flat = np.full((41, 41), 77, np.uint8)
    r = R.vifp(flat, R.img_pair(np.random.default_rng(1), 41, 41, 1)[0], 0, R.CHANNELS)
    assert r["den"] == [0.0] * 4 and math.isnan(r["value"])


def test_entry_point_refuses_before_any_device_call():
    """With a null context every valid argument list ends in 'null or destroyed context'; every refusal below comes first."""
    lib = _native.load()
    out = (_native.VifScale * 4)()
    buf = C.create_string_buffer(16)
    p = C.cast(buf, C.c_void_p)

    def call(a=p, sa=192, b=p, sb=192, h=50, w=64, cn=3, cb=4, mode=R.Y, o=out):
        rc = lib.sr_vif_u8(None, a, sa, b, sb, h, w, cn, cb, mode, o)
        return rc, _native.last_error()

    for kw in (dict(), dict(mode=R.Y_ROUND), dict(cn=1, sa=64, sb=64, mode=R.CHANNELS), dict(h=49)):     # 49 - 8 = 41: fine
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg, kw
    for kw in (dict(a=None), dict(b=None), dict(o=None)):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and "null argument" in msg, kw
    for kw, word in ((dict(cn=2), "channels"), (dict(cn=4), "channels"), (dict(cn=1, sa=64, sb=64), "Y modes"),
                     (dict(cn=1, sa=64, sb=64, mode=R.Y_ROUND), "Y modes"), (dict(mode=R.CHANNELS), "one gray plane"),
                     (dict(mode=3), "mode"), (dict(mode=-1), "mode"), (dict(cb=-1), "crop_border"), (dict(h=0), "h, w")):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and word in msg, (kw, msg)
    for kw, word in ((dict(sa=191), "stride"), (dict(sb=191), "stride"), (dict(cn=1, mode=0, sa=63, sb=64), "stride"),
                     (dict(h=48), "at least 41"), (dict(w=48, sa=144, sb=144), "at least 41"), (dict(cb=5), "at least 41"),
                     (dict(cb=1000), "at least 41")):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_SHAPE and word in msg, (kw, msg)


def test_module_methods_refuse_before_any_device_call():
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()

    def no_device():
        raise AssertionError("the device context was asked for")
    q._ctx = no_device
    a = np.zeros((50, 64, 3), np.uint8)
    g = np.zeros((50, 64), np.uint8)
    with pytest.raises(NotImplementedError):
        q.calculate_vif(a.astype(np.float32), a)
    with pytest.raises(NotImplementedError):
        q.calculate_vif(a, a.astype(np.uint16))
    for x, y in ((a, a[:49]), (a, a[:, :63]), (a, g), (a[:, :, :1], g)):     # no common rectangle is taken
        with pytest.raises(ValueError, match="same shape"):
            q.calculate_vif(x, y)
    with pytest.raises(ValueError, match="3 channels"):
        q.calculate_vif(np.zeros((50, 64, 4), np.uint8), np.zeros((50, 64, 4), np.uint8))
    with pytest.raises(ValueError, match="luma only"):
        q.calculate_vif(a, a, test_y_channel=False)
    with pytest.raises(ValueError, match="y_round"):
        q.calculate_vif(g, g, y_round=True)
    with pytest.raises(ValueError, match="at least 41"):
        q.calculate_vif(a, a, crop_border=5)
    with pytest.raises(ValueError, match="crop_border"):
        q.calculate_vif(a, a, crop_border=-1)
    with pytest.raises(ValueError):
        q.calculate_vif(a, a, crop_border=1.5)
    # the device form
    with pytest.raises(ValueError, match="same shape"):
        q.calculate_vif_device(256, (50, 64, 3), 256, (50, 60, 3))
    with pytest.raises(ValueError, match="null"):
        q.calculate_vif_device(0, (50, 64, 3), 256, (50, 64, 3))
    with pytest.raises(_native.SrShapeError, match="stride"):
        q.calculate_vif_device(256, (50, 64, 3), 256, (50, 64, 3), stride2=191)
    with pytest.raises(ValueError, match="at least 41"):
        q.calculate_vif_device(256, (50, 64, 3), 256, (50, 64, 3), crop_border=5)
    # a valid call gets as far as the context, and no further: colour on its luma, gray as it is
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_vif(a, a, crop_border=4)
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_vif(g, g)
    with pytest.raises(AssertionError, match="device context"):
        q.calculate_vif_device(256, (50, 64), 256, (50, 64), stride1=80)
    # the pipeline options are off by default
    import main as sr_main
    assert sr_main.PipelineConfig().qa_vif is False and sr_main.PipelineConfig().qa_gmsd is False


def test_restatement_basics():
    rng = np.random.default_rng(3)
    a, b = R.img_pair(rng, 64, 80, 3)
    r = R.vifp(a, b)
    assert all(d > 0 for d in r["den"]) and 0.05 < r["value"] < 0.95
    # not symmetric
    assert abs(R.vifp(b, a)["value"] - r["value"]) > 1e-5
    # identical seeded noise: within 1e-11 of 1, not exactly 1
    n = rng.integers(0, 256, (64, 80), dtype=np.uint8)
    v = R.vifp(n, n, 0, R.CHANNELS)["value"]
    assert abs(v - 1.0) <= 1e-11 and v != 1.0
    # the three planes are told apart, and the crop
    vals = {R.vifp(a, b, 0, m)["value"] for m in (R.Y, R.Y_ROUND)} | {R.vifp(a[..., 1], b[..., 1], 0, R.CHANNELS)["value"],
                                                                     R.vifp(a, b, 1)["value"]}
    assert len(vals) == 4
    # the separable form the kernel uses stays three orders below the 1e-9 bar
    x, y = R.plane(a, R.Y), R.plane(b, R.Y)
    t = _native.vif_window(1)
    sep = lambda p: sum(t[k] * sum(t[j] * p[k:k + 48, j:j + 64] for j in range(17)) for k in range(17))
    mu1 = sep(x)
    s1 = np.maximum(sep(x * x) - mu1 * mu1, 0.0)
    s1[s1 < 1e-10] = 0.0
    den1 = np.log10(1.0 + s1 / 2.0).sum()
    assert abs(den1 - r["den"][0]) <= 1e-12 * r["den"][0]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_restatement_kills_mutants(mutant):
    """Each plausible misreading of the definition moves the restatement's own answer by more than 1e-6 relative."""
    rng = np.random.default_rng(17)
    for h, w in ((110, 97), (97, 130)):         # the previous scale's window leaves scale 4 a map from 97 on
        a, b = R.img_pair(rng, h, w, 3)
        good, bad = R.vifp(a, b), R.vifp(a, b, mutant=mutant)
        rel = abs(bad["value"] - good["value"]) / abs(good["value"])
        print(mutant, h, w, good["value"], bad["value"], rel)
        assert rel > 1e-6, (mutant, h, w)
        moved = [abs(x - y) / abs(y) for x, y in zip(bad["num"][1:], good["num"][1:])]
        assert max(moved) > 1e-6


def test_tall_periodic_form_is_the_direct_restatement():
    """R.vifp_tall (the reference of the GPU suite's tall images) against the direct 2-D evaluation, at heights that leave
    every scale a remainder; only the order of the final additions differs."""
    rng = np.random.default_rng(29)
    for cn, mode in ((1, R.CHANNELS), (3, R.Y)):
        blk_a, blk_b = R.img_pair(rng, 104, 41, cn)
        for h in (312, 477, 1003):
            direct = R.vifp(R.tile_rows(blk_a, h), R.tile_rows(blk_b, h), 0, mode)
            tall = R.vifp_tall(blk_a, blk_b, h, mode)
            assert tall["count"] == direct["count"] and [tuple(x) for x in direct["sizes"]] == tall["sizes"]
            for k in ("num", "den"):
                for s in range(4):
                    assert tall[k][s] == pytest.approx(direct[k][s], rel=1e-13, abs=0), (cn, h, k, s)
    # a period that is no multiple of 8 is refused
    with pytest.raises(AssertionError):
        R.vifp_tall(blk_a[:100], blk_b[:100], 400, R.Y)
