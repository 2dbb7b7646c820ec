"""CPU: the host side of the SR-benchmark PSNR / SSIM (sr_bench_plan, every refusal of sr_bench_u8 and of the module methods
before a device call, the pipeline option's default) and the NumPy restatement tests/_srbench_ref.py against the scikit-image
fixture."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _native
import _srbench_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
MODES = (_native.BENCH_CHANNELS, _native.BENCH_Y, _native.BENCH_Y_ROUND)


def test_modes_are_the_header_enum():
    assert (_native.BENCH_CHANNELS, _native.BENCH_Y, _native.BENCH_Y_ROUND) == (R.CHANNELS, R.Y, R.Y_ROUND) == (0, 1, 2)
    text = open(os.path.join(os.path.dirname(GOLD), "..", "include", "sr_hip.h")).read()
    assert "enum sr_bench_mode { SR_BENCH_CHANNELS = 0, SR_BENCH_Y = 1, SR_BENCH_Y_ROUND = 2 }" in text
    assert C.sizeof(_native.BenchSums) == 32
    # the contract's words on parity stand in the header
    assert "PARITY UNPINNED with BasicSR" in text and "float32" in text


def test_plan_sizes_and_counts_against_closed_forms():
    for h, w in ((11, 11), (19, 27), (96, 120), (300, 600), (11550, 17320)):
        for cb in (0, 1, 3, 4):
            for cn in (1, 3):
                for mode in MODES:
                    if mode != _native.BENCH_CHANNELS and cn == 1:
                        continue
                    ch, cw = h - 2 * cb, w - 2 * cb
                    if min(ch, cw) < 11:
                        with pytest.raises(_native.SrShapeError, match=r"at least 11\b"):
                            _native.bench_plan(h, w, cn, cb, mode)
                        with pytest.raises(ValueError):
                            R.plan(h, w, cn, cb, mode)
                        continue
                    planes = cn if mode == _native.BENCH_CHANNELS else 1
                    p = _native.bench_plan(h, w, cn, cb, mode)
                    assert p["size"] == (ch, cw), (h, w, cb)
                    assert p["n_elems"] == ch * cw * planes and p["n_map"] == (ch - 10) * (cw - 10) * planes
                    assert (ch, cw, p["n_elems"], p["n_map"]) == R.plan(h, w, cn, cb, mode)
                    # two doubles per block of at most 246 x 128 map samples (at least 246 x 16), plus small reduction buffers
                    blocks_min = -(-(ch - 10) // 128) * -(-(cw - 10) // 246) * planes
                    blocks_max = -(-(ch - 10) // 16) * -(-(cw - 10) // 246) * planes
                    assert 16 * blocks_min <= p["scratch_bytes"] <= 16 * blocks_max + 3 * 256 + (1 << 16), (h, w, cb, p)
    assert _native.bench_plan(11, 11, 3, 0, _native.BENCH_Y)["n_map"] == 1
    p = _native.bench_plan(19, 31, 3, 4, _native.BENCH_CHANNELS)
    assert (p["size"], p["n_elems"], p["n_map"]) == ((11, 23), 11 * 23 * 3, 13 * 3)
    lib = _native.load()
    assert lib.sr_bench_plan(64, 64, 3, 2, 1, None, None, None, None, None) == _native.SR_OK            # outputs may be NULL


def test_plan_refusals():
    for kw, word in ((dict(cn=2), "channels"), (dict(cn=4), "channels"), (dict(cn=0), "channels"), (dict(mode=3), "mode"),
                     (dict(mode=-1), "mode"), (dict(cn=1, mode=_native.BENCH_Y), "Y modes"),
                     (dict(cn=1, mode=_native.BENCH_Y_ROUND), "Y modes"), (dict(crop_border=-1), "crop_border"),
                     (dict(h=0), "h, w"), (dict(w=-5), "h, w")):
        args = dict(h=64, w=64, cn=3, crop_border=2, mode=_native.BENCH_Y)
        args.update(kw)
        with pytest.raises(ValueError, match=word) as e:
            _native.bench_plan(**args)
        assert not isinstance(e.value, _native.SrShapeError), kw
    for h, w, cb in ((10, 64, 0), (64, 10, 0), (18, 64, 4), (64, 18, 4), (8, 8, 4), (8, 8, 40)):
        with pytest.raises(_native.SrShapeError, match=r"at least 11\b"):
            _native.bench_plan(h, w, 3, cb)
    with pytest.raises(ValueError):
        _native.bench_plan(64, 64, 3, 1.5)
    _native.bench_plan(19, 19, 3, 4)                                       # exactly 11 left


def test_entry_point_refuses_before_any_device_call():
    """With a null context every valid argument list ends in 'null or destroyed context'; every refusal below comes first."""
    lib = _native.load()
    out = _native.BenchSums()
    buf = C.create_string_buffer(16)
    p = C.cast(buf, C.c_void_p)

    def call(a=p, sa=192, b=p, sb=192, h=40, w=64, cn=3, cb=4, mode=_native.BENCH_Y, dr=255.0, o=C.byref(out)):
        rc = lib.sr_bench_u8(None, a, sa, b, sb, h, w, cn, cb, mode, dr, o)
        return rc, _native.last_error()

    rc, msg = call()
    assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg
    for mode in MODES:
        rc, msg = call(mode=mode)
        assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg
    rc, msg = call(cn=1, sa=64, sb=64, mode=_native.BENCH_CHANNELS)
    assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg
    for kw in (dict(a=None), dict(b=None), dict(o=None)):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and "null argument" in msg, kw
    for kw, word in ((dict(cn=2), "channels"), (dict(cn=4), "channels"), (dict(cn=1, sa=64, sb=64), "Y modes"),
                     (dict(cn=1, sa=64, sb=64, mode=_native.BENCH_Y_ROUND), "Y modes"), (dict(mode=3), "mode"), (dict(mode=-1), "mode"),
                     (dict(cb=-1), "crop_border"), (dict(dr=0.0), "data_range"), (dict(dr=-1.0), "data_range"),
                     (dict(dr=float("inf")), "data_range"), (dict(dr=float("nan")), "data_range"), (dict(h=0), "h, w")):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_INVALID_ARG and word in msg, (kw, msg)
    for kw, word in ((dict(sa=191), "stride"), (dict(sb=191), "stride"), (dict(cn=1, mode=0, sa=63, sb=64), "stride"),
                     (dict(h=18), "at least 11"), (dict(w=18, sa=54, sb=54), "at least 11"), (dict(cb=15), "at least 11"),
                     (dict(cb=1000), "at least 11")):
        rc, msg = call(**kw)
        assert rc == _native.SR_ERR_SHAPE and word in msg, (kw, msg)
    rc, msg = call(h=19)
    assert rc == _native.SR_ERR_INVALID_ARG and "context" in msg              # 19 - 8 = 11: fine


def test_module_methods_refuse_before_any_device_call():
    import quality_assessment_module as qam
    q = qam.QualityAssessmentModule()

    def no_device():
        raise AssertionError("the device context was asked for")
    q._ctx = no_device
    a = np.zeros((40, 64, 3), np.uint8)
    g = np.zeros((40, 64), np.uint8)
    with pytest.raises(NotImplementedError):
        q.evaluate_sr_benchmark(a.astype(np.float32), a)
    with pytest.raises(NotImplementedError):
        q.evaluate_sr_benchmark(a, a.astype(np.uint16))
    for x, y in ((a, a[:39]), (a, a[:, :63]), (a, g), (a[:, :, :1], g)):     # no common rectangle is taken
        with pytest.raises(ValueError, match="same shape"):
            q.evaluate_sr_benchmark(x, y)
    with pytest.raises(ValueError, match="3 channels"):
        q.evaluate_sr_benchmark(np.zeros((40, 64, 4), np.uint8), np.zeros((40, 64, 4), np.uint8), test_y_channel=False)
    with pytest.raises(ValueError, match="test_y_channel"):
        q.evaluate_sr_benchmark(g, g)                                        # Y needs RGB
    with pytest.raises(ValueError, match="y_round"):
        q.evaluate_sr_benchmark(a, a, test_y_channel=False, y_round=True)
    with pytest.raises(ValueError, match="at least 11"):
        q.evaluate_sr_benchmark(a, a, crop_border=15)
    with pytest.raises(ValueError, match="crop_border"):
        q.evaluate_sr_benchmark(a, a, crop_border=-1)
    with pytest.raises(ValueError):
        q.evaluate_sr_benchmark(a, a, crop_border=1.5)
    for dr in (0.0, -255.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="data_range"):
            q.evaluate_sr_benchmark(a, a, data_range=dr)
    # the device form
    with pytest.raises(ValueError, match="same shape"):
        q.evaluate_sr_benchmark_device(256, (40, 64, 3), 256, (40, 60, 3))
    with pytest.raises(ValueError, match="null"):
        q.evaluate_sr_benchmark_device(0, (40, 64, 3), 256, (40, 64, 3))
    with pytest.raises(ValueError, match="at least 11"):
        q.evaluate_sr_benchmark_device(256, (40, 64, 3), 256, (40, 64, 3), crop_border=16)
    with pytest.raises(ValueError, match="test_y_channel"):
        q.evaluate_sr_benchmark_device(256, (40, 64), 256, (40, 64))
    # a valid call gets as far as the context, and no further
    with pytest.raises(AssertionError, match="device context"):
        q.evaluate_sr_benchmark(a, a, crop_border=4)
    with pytest.raises(AssertionError, match="device context"):
        q.evaluate_sr_benchmark_device(256, (40, 64), 256, (40, 64), test_y_channel=False)
    # the pipeline option is off by default
    import main as sr_main
    assert sr_main.PipelineConfig().qa_benchmark is False


def test_bench_values():
    rec = {"sse": 65025 * 100, "ssim_sum": 30.0, "n_elems": 100, "n_map": 40}
    psnr, ssim = _native.bench_values(rec)
    assert psnr == pytest.approx(0.0, abs=1e-12) and ssim == 0.75
    assert _native.bench_values({**rec, "sse": 0}) == (math.inf, 0.75)
    assert _native.bench_values({**rec, "sse": 100.0}, data_range=10.0)[0] == pytest.approx(20.0, abs=1e-12)


def test_restatement_matches_skimage():
    z = np.load(os.path.join(GOLD, "srbench_skimage.npz"))
    a, b = z["a"], z["b"]
    assert a.shape == b.shape == (96, 120, 3) and a.dtype == np.uint8 and str(z["skimage_version"]) == "0.18.3"
    assert z["crop_borders"].tolist() == [0, 4]
    a2, b2 = R.img_pair(np.random.default_rng(20260519), 96, 120, 3)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)
    seen = []
    for i, cb in enumerate((0, 4)):
        for mode, name in ((R.Y, "y"), (R.Y_ROUND, "y_round"), (R.CHANNELS, "rgb")):
            r = R.bench(a, b, cb, mode)
            print(cb, name, r["psnr"], float(z["psnr_" + name][i]), r["ssim"], float(z["ssim_" + name][i]))
            assert r["psnr"] == pytest.approx(float(z["psnr_" + name][i]), rel=1e-13, abs=0)
            assert r["ssim"] == pytest.approx(float(z["ssim_" + name][i]), rel=1e-13, abs=0)
            seen.append((r["psnr"], r["ssim"]))
    # the three modes and the two crops are told apart
    assert len(set(seen)) == 6
    assert all(abs(p1 - p2) > 1e-4 and abs(s1 - s2) > 1e-5 for k, (p1, s1) in enumerate(seen) for (p2, s2) in seen[k + 1:])


def test_restatement_planes():
    rnd = np.random.default_rng(11)
    img = rnd.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    x = R.x_int(img)
    assert x.min() >= 4080000 and x.max() <= 59925000 < 1 << 26
    white, black = np.full((1, 1, 3), 255, np.uint8), np.zeros((1, 1, 3), np.uint8)
    assert R.x_int(white)[0, 0] == 59925000 and R.x_int(black)[0, 0] == 4080000
    assert R.y_round(white)[0, 0] == 235 and R.y_round(black)[0, 0] == 16
    # half up: X / 255000 = k + 0.5 exactly must go to k + 1
    y = R.y_round(img)
    assert np.array_equal(y, np.floor(x / 255000.0 + 0.5).astype(np.uint8))
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(R.gray_as_y_round(v), R.y_round(np.stack([v, v, v], -1)))
    assert R.blocks(26, 256) == (1, 1) and R.blocks(27, 257) == (2, 2) and R.blocks(11, 11) == (1, 1)
